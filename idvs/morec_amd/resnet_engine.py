"""Host-side orchestration of the ResNet item tower: explicit forward and hand-derived backward of ``Resnet_Encoder.forward``
(``V/model/encoders.py:34-41``) = ``GELU(image_net(x))`` with ``image_net`` a torchvision ``ResNet`` whose ``fc`` was replaced by
``Linear(num_fc_ftr, embedding_dim)`` (``V/run.py:38-46``; the reference selects it by ``'resnet' in CV_model_load``,
``V/model/model.py:24-25``).

Layout: activations are NHWC, viewed as ``[N H W, C]`` rows in the compute dtype, so every convolution is an "NT" product over rows.
A 1 x 1 stride-1 convolution IS ``ops.gemm_nt`` on the activation matrix; a 1 x 1 stride-2 convolution (the downsample branch) is a row
subsample (``morec_im2col_nhwc`` with one tap) followed by ``gemm_nt``; 3 x 3 and 7 x 7 run the implicit-GEMM kernel of ``csrc/conv.hip``,
whose gather form is the data gradient.  ``state_dict`` keeps torchvision's OIHW weights; ``resnet_prepare`` permutes them to
``[Cout, KH, KW, Cin]`` (and ``[Cin, KH, KW, Cout]`` for the data gradient) once per call and the backward permutes the gradient back.

Weight gradients of the k x k layers: ``morec_im2col_nhwc`` over a range of images, then the library's weight-gradient GEMM, chunked so
that the im2col workspace stays under ``WGRAD_WS_CAP`` bytes.  Correctness first: a fused gather + weight-gradient kernel is not built.

BatchNorm2d in training mode uses the statistics of ALL rows of the call (the zero images of padding items included, as in the
reference), so the training forward never chunks the batch; the statistics are per-slab ``(count, mean, M2)`` partials merged in slab
order (``merge_bn_partials``).  Evaluation mode applies the running statistics through the same apply kernel.  A frozen gamma / beta
still normalises with batch statistics in training mode: it only gets no gradient buffer.

Synchronised BatchNorm (``BnSync``: a process group and its size; ``None`` is the plain path, untouched).  Training mode with W ranks is
BatchNorm over the concatenation of the ranks' rows, as torch documents ``SyncBatchNorm``.  Forward: stats -> the rank's own slabs merged
-> one all-gather of the [3, C] results, rank-major -> ``morec_bn_merge`` over those W partials in rank order, which also updates the
running statistics with the global count.  Backward: the local sums (d gamma and d beta stay LOCAL: DDP averages them like every other
parameter gradient) -> one all-gather of [2, C] -> ``morec_bn_bwd_fold`` in rank order -> the apply kernel that divides by the merged
count row it reads on the device.  An all-gather and a fixed-order fold, never an all-reduce: every rank computes the same bits, and the
host never learns the global row count.  One collective per BatchNorm forward and one per backward (53 + 53 at ResNet-50), all on the
current stream.  Whether a BatchNorm communicates follows from configuration alone (training flag, sync context, the frozen prefix), never
from data: every rank issues the same collectives in the same order.  Evaluation mode has none."""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

from . import engine, ops
from .engine import _splitk, linear_wgrad_, prepare_linear

IN = "image_net."
_CONV_TN_WS = {}      # slab workspace of conv_wgrad's GEMMs: they run on the CURRENT stream while engine.linear_wgrad_'s run on the
                      # weight-gradient stream with ops._TN_WS -- one workspace per stream, or two launches would overwrite each other's slabs
WGRAD_WS_CAP = 256 << 20      # bytes of im2col workspace per weight-gradient chunk (ResNet-50, fp16, layer1: 71 images of 224 x 224 a chunk)


def merge_bn_partials(part: torch.Tensor) -> torch.Tensor:
    """``part`` [slabs, 3, C] = (count, mean, M2) per slab and channel -> [3, C], merged in slab order with Chan's formula
    (``mean += delta nb / n``, ``M2 += M2b + delta^2 na nb / n``) in the dtype of ``part``.  Device tensors run ``morec_bn_merge`` (the
    same arithmetic, one thread per channel); host tensors run it here.  ``merge_bn_over_ranks`` runs it over the gathered [3, C] results of the ranks, in rank order."""
    if part.is_cuda:
        return ops.bn_merge(part.contiguous(), 0.0, need_merged=True)[2]
    n, mean, m2 = part[0, 0].clone(), part[0, 1].clone(), part[0, 2].clone()
    for s in range(1, part.shape[0]):
        nb, mb, m2b = part[s, 0], part[s, 1], part[s, 2]
        tot, delta = n + nb, mb - mean
        mean = mean + delta * (nb / tot)
        m2 = m2 + m2b + delta * delta * (n * nb / tot)
        n = tot
    return torch.stack([n, mean, m2])


class BnSync(NamedTuple):
    """The sync context of the BatchNorm layers: ``group`` (a ``torch.distributed`` process group; None: the world) of ``world`` ranks."""
    group: Any
    world: int


def gather_over_ranks(t: torch.Tensor, sync: BnSync) -> torch.Tensor:
    """[k, C] of every rank -> [W, k, C], rank-major (one all-gather; host tensors too)."""
    from .functional import _all_gather_cat
    return _all_gather_cat(t.unsqueeze(0).contiguous(), sync.world, group=sync.group)


def merge_bn_over_ranks(merged: torch.Tensor, sync: BnSync) -> torch.Tensor:
    """A rank's own merged [3, C] -> the [3, C] of all ranks' rows: gathered, then ``merge_bn_partials`` over the W partials in rank
    order.  The same bits on every rank."""
    return merge_bn_partials(gather_over_ranks(merged, sync))


def fold_bn_sums_over_ranks(sums: torch.Tensor, sync: BnSync) -> torch.Tensor:
    """A rank's backward sums [2, C] -> the sums over all ranks, added in rank order (``morec_bn_bwd_fold``; a host loop for host
    tensors)."""
    parts = gather_over_ranks(sums, sync)
    if parts.is_cuda:
        return ops.bn_bwd_fold(parts)
    total = torch.zeros_like(parts[0])
    for r in range(parts.shape[0]):
        total = total + parts[r]
    return total


def conv_names(shape, prefix: str = IN):
    """[(weight name, KH, stride, pad)] of every convolution, in registration order."""
    out = [(prefix + "conv1.weight", 7, 2, 3)]
    for name, _, _, stride, down in shape.blocks():
        B = prefix + name + "."
        if shape.block == "basic":
            out += [(B + "conv1.weight", 3, stride, 1), (B + "conv2.weight", 3, 1, 1)]
        else:
            out += [(B + "conv1.weight", 1, 1, 0), (B + "conv2.weight", 3, stride, 1), (B + "conv3.weight", 1, 1, 0)]
        if down:
            out.append((B + "downsample.0.weight", 1, stride, 0))
    return out


def resnet_prepare(p: dict, shape, dtype, prefix: str = IN, need_grad: bool = True, features_only: bool = False):
    """Compute-dtype copies of the weights in the kernels' layouts: ``w`` [Cout, KH, KW, Cin], ``wt`` [Cin, KH, KW, Cout] (the data
    gradient's; not for the stem, whose input takes no gradient)."""
    prep = {}
    for i, (name, k, stride, pad) in enumerate(conv_names(shape, prefix)):
        w = p[name].detach().permute(0, 2, 3, 1).contiguous()
        w = w if w.dtype == dtype else ops.cast(w, dtype)
        wt = w.permute(3, 1, 2, 0).contiguous() if (need_grad and i > 0) else None
        prep[name] = (w, wt, k, stride, pad)
    if not features_only:
        prep["fc"] = prepare_linear(p[prefix + "fc.weight"], dtype)
    return prep


# ---------------------------------------------------------------------------------------------------------
def _conv_fwd(x, geom, cw):
    """x [N H W, Cin] -> (out [N Ho Wo, Cout], (N, Ho, Wo), the matrix the weight gradient multiplies (1 x 1) or None)."""
    w, _, k, stride, pad = cw
    N, H, W = geom
    Ho, Wo = ops.conv_out_size(H, k, stride, pad), ops.conv_out_size(W, k, stride, pad)
    if k == 1:
        xs = x if stride == 1 else ops.im2col_nhwc(x, N, H, W, 1, 1, stride, 0)
        return ops.gemm_nt(xs, w.view(w.shape[0], -1)), (N, Ho, Wo), xs
    return ops.conv2d_fwd(x, w, N, H, W, stride, pad), (N, Ho, Wo), None


def conv_wgrad(dy, x, geom, k, stride, pad, chunk_images=None):
    """fp32 [Cout, KH, KW, Cin] = the weight gradient of a k x k convolution: im2col of a range of images, then the weight-gradient
    GEMM accumulating into one buffer, chunk after chunk on the current stream.  ``chunk_images``: images per chunk (default: as many
    as keep the im2col workspace under ``WGRAD_WS_CAP``)."""
    N, H, W = geom
    Cin, Cout = x.shape[1], dy.shape[1]
    Ho, Wo = ops.conv_out_size(H, k, stride, pad), ops.conv_out_size(W, k, stride, pad)
    K = k * k * Cin
    ev = 16 // x.element_size()
    ld = (K + ev - 1) // ev * ev
    if chunk_images is None:
        chunk_images = max(1, WGRAD_WS_CAP // (Ho * Wo * ld * x.element_size()))
    g = torch.zeros((Cout, ld), device=x.device, dtype=torch.float32)
    direct = ops.is16(x.dtype) and Cout % 8 == 0 and ld % 8 == 0
    for n0 in range(0, N, chunk_images):
        r0, r1 = n0 * Ho * Wo, min(N, n0 + chunk_images) * Ho * Wo
        col = ops.im2col_nhwc(x, N, H, W, k, k, stride, pad, r0, r1, ld)
        dyc = dy[r0:r1]
        if direct:
            ops.gemm_tn_(dyc, col, g, split_m=_splitk(Cout, ld, r1 - r0), accumulate=True, ws_cache=_CONV_TN_WS)
        else:      # fp32 storage: transposed copies and the NT product, one writer per element
            ops.gemm_nt(ops.transpose(dyc), ops.transpose(col), out=g, accumulate=1)
    return g[:, :K].view(Cout, k, k, Cin)


def _conv_bwd(dy, x, xs, geom, cw, gw, need_dx, chunk_images=None):
    """``gw``: the fp32 OIHW gradient buffer (None: frozen).  Returns dx [N H W, Cin] or None."""
    w, wt, k, stride, pad = cw
    N, H, W = geom
    if gw is not None:
        if k == 1:
            linear_wgrad_(dy, xs, gw.view(gw.shape[0], -1))
        else:
            gw.add_(conv_wgrad(dy, x, geom, k, stride, pad, chunk_images).permute(0, 3, 1, 2))
    if not need_dx:
        return None
    if k == 1 and stride == 1:
        return ops.gemm_nt(dy, wt.view(wt.shape[0], -1))
    return ops.conv2d_bwd_data(dy, wt, N, H, W, stride, pad)


def _bn_fwd(p, bufs, name, x, training, relu, res=None, sync=None):
    """BatchNorm2d ``name`` over x [rows, C] (+ residual, ReLU) -> (y, (mean, rstd, count)); ``count``: the merged count row of all
    ranks' rows under ``sync`` in training mode (what the backward divides by), else None."""
    rm, rv = bufs[name + ".running_mean"], bufs[name + ".running_var"]
    count = None
    if training and sync is not None:
        parts = gather_over_ranks(ops.bn_merged(ops.bn_stats(x)), sync)
        mean, rstd, merged = ops.bn_merge(parts, p["eps"], rm, rv, p["momentum"], need_merged=True)
        count = merged[0]
        bufs[name + ".num_batches_tracked"].add_(1)
    elif training:
        mean, rstd, _ = ops.bn_merge(ops.bn_stats(x), p["eps"], rm, rv, p["momentum"])
        bufs[name + ".num_batches_tracked"].add_(1)
    else:
        mean, rstd = rm, ops.bn_rstd(rv, p["eps"])
    y = ops.bn_apply_fwd(x, mean, rstd, p[name + ".weight"], p[name + ".bias"], res=res, relu=relu)
    return y, (mean, rstd, count)


def _bn_bwd(p, grads, name, dy, y_relu, x, stat, training, need_dz=False, sync=None):
    """-> (dx, dz).  ``y_relu``: the BatchNorm's saved output when a ReLU follows it, else None.  ``stat``: ``_bn_fwd``'s."""
    mean, rstd, count = stat
    sums = ops.bn_bwd_reduce(dy, y_relu, x, mean, rstd)
    if name + ".weight" in grads:
        grads[name + ".weight"].copy_(sums[1])
    if name + ".bias" in grads:
        grads[name + ".bias"].copy_(sums[0])
    if training and sync is not None:
        return ops.bn_bwd_apply(dy, y_relu, x, mean, rstd, p[name + ".weight"], fold_bn_sums_over_ranks(sums, sync), need_dz=need_dz,
                                count=count)
    return ops.bn_bwd_apply(dy, y_relu, x, mean, rstd, p[name + ".weight"], sums if training else None, need_dz=need_dz)


def resnet_forward(p: dict, bufs: dict, prep, shape, pixels: torch.Tensor, dtype, need_grad: bool, prefix: str = IN, training: bool = False,
                   features_only: bool = False, sync=None):
    """pixels fp32 [n_img, 3, H, W] (normalised) or uint8 [n_img, H, W, 3] (decoded) -> item vectors [n_img, D]
    (``GELU(fc(avgpool(layer4(...))))``).  ``bufs``: the BatchNorm buffers by name (training mode updates them in place).
    ``features_only``: return ``(pooled [n_img, num_fc_ftr], None)``, the input of ``fc``.  ``sync``: a ``BnSync`` -- training mode takes
    the BatchNorm statistics over every rank's rows (under ``no_grad`` too); None: this call's rows alone."""
    q = dict(p)
    q["eps"], q["momentum"] = shape.eps, shape.momentum
    u8 = pixels.dtype == torch.uint8
    N, H, W = (pixels.shape[0], pixels.shape[1], pixels.shape[2]) if u8 else (pixels.shape[0], pixels.shape[2], pixels.shape[3])
    src, ids = engine.image_source(pixels)      # ImageIds: the conversion reads the device catalogue's rows through the ids
    x0 = ops.pixels_to_nhwc(src, dtype, ids=ids)
    tape = []
    c0, g1, _ = _conv_fwd(x0, (N, H, W), prep[prefix + "conv1.weight"])
    y0, s0 = _bn_fwd(q, bufs, prefix + "bn1", c0, training, True, sync=sync)
    x, idx = ops.maxpool3x3s2_fwd(y0, *g1)
    geom = (N, (g1[1] - 1) // 2 + 1, (g1[2] - 1) // 2 + 1)
    stem = (x0, (N, H, W), c0, y0, s0, g1, idx)
    n_conv = 2 if shape.block == "basic" else 3
    for name, _, _, stride, down in shape.blocks():
        B = prefix + name + "."
        rec = dict(name=B, x=x, geom=geom, convs=[], down=None)
        h, hg = x, geom
        for i in range(1, n_conv + 1):
            cw = prep[B + f"conv{i}.weight"]
            c, cg, xs = _conv_fwd(h, hg, cw)
            last = i == n_conv
            if last:
                ident = x
                if down:
                    dc, _, dxs = _conv_fwd(x, geom, prep[B + "downsample.0.weight"])
                    ident, ds = _bn_fwd(q, bufs, B + "downsample.1", dc, training, False, sync=sync)
                    rec["down"] = (dxs, dc, ds)
                y, st = _bn_fwd(q, bufs, B + f"bn{i}", c, training, True, res=ident, sync=sync)
            else:
                y, st = _bn_fwd(q, bufs, B + f"bn{i}", c, training, True, sync=sync)
            rec["convs"].append((h, xs, hg, c, y, st))
            h, hg = y, cg
        tape.append(rec)
        x, geom = h, hg
    pooled = ops.swin_pool_fwd(x, N, geom[1] * geom[2])
    if features_only:
        return pooled, None
    item, pre = engine.head_forward(pooled, prep["fc"], p[prefix + "fc.bias"], need_grad)
    saved = (shape, stem, tape, geom, pooled, pre, training, sync) if need_grad else None
    return item, saved


def resnet_backward(p: dict, prep, saved, d_item: torch.Tensor, grads: dict, prefix: str = IN, chunk_images=None):
    """grads: name -> fp32 buffer (zeroed; accumulated into).  A name that is missing from ``grads`` is frozen: a convolution without a
    buffer skips its weight gradient, a BatchNorm without one only skips its own gamma / beta gradient.  Under a sync context every
    BatchNorm that is walked gathers once; which ones are walked follows from the names in ``grads`` (configuration, the same on every
    rank)."""
    shape, stem, tape, geom, pooled, pre, training, sync = saved
    n_conv = 2 if shape.block == "basic" else 3
    dpooled = engine.head_backward(d_item, pre, pooled, prep["fc"], grads.get(prefix + "fc.weight"), grads.get(prefix + "fc.bias"), pooled.shape[1])
    dout = ops.swin_pool_bwd(dpooled, geom[0], geom[1] * geom[2])
    # the backward ends at the lowest block that holds a trainable parameter (``--freeze_paras_before``: the frozen prefix is not walked)
    lowest = min((i for i, rec in enumerate(tape) if any(n.startswith(rec["name"]) for n in grads)), default=len(tape))
    stem_trains = any(n.startswith((prefix + "conv1.", prefix + "bn1.")) for n in grads)
    for i_rec in range(len(tape) - 1, -1, -1):
        rec = tape[i_rec]
        if not stem_trains and i_rec < lowest:
            return
        B = rec["name"]
        d, dz = dout, None
        for i in range(n_conv, 0, -1):
            h, xs, hg, c, y, st = rec["convs"][i - 1]
            last = i == n_conv
            d, dzi = _bn_bwd(p, grads, B + f"bn{i}", d, y, c, st, training, need_dz=last, sync=sync)
            if last:
                dz = dzi
            d = _conv_bwd(d, h, xs, hg, prep[B + f"conv{i}.weight"], grads.get(B + f"conv{i}.weight"), True, chunk_images)
        if rec["down"] is not None:
            dxs, dc, ds = rec["down"]
            dd, _ = _bn_bwd(p, grads, B + "downsample.1", dz, None, dc, ds, training, sync=sync)
            dz = _conv_bwd(dd, rec["x"], dxs, rec["geom"], prep[B + "downsample.0.weight"], grads.get(B + "downsample.0.weight"), True,
                           chunk_images)
        dout = ops.scaled_sum([d, dz], 1.0)
    if not stem_trains:
        return
    x0, g0, c0, y0, s0, g1, idx = stem
    dy0 = ops.maxpool3x3s2_bwd(dout, idx, *g1)
    dc0, _ = _bn_bwd(p, grads, prefix + "bn1", dy0, y0, c0, s0, training, sync=sync)
    _conv_bwd(dc0, x0, None, g0, prep[prefix + "conv1.weight"], grads.get(prefix + "conv1.weight"), False, chunk_images)      # pixels take no gradient


TOWER = engine.Tower(
    prepare=lambda p, c, need_grad: resnet_prepare(p, c.shape, c.dtype, c.prefix, need_grad=need_grad, features_only=c.features_only),
    plan=engine.no_plan,
    forward=lambda p, prep, x, c, need_grad: resnet_forward(p, c.kw["bufs"], prep, c.shape, x, c.dtype, need_grad, c.prefix, c.training,
                                                            features_only=c.features_only, sync=c.kw["sync"]),
    backward=lambda p, prep, saved, d, grads, c: resnet_backward(p, prep, saved, d, grads, c.prefix),
    # a frozen parameter gets no buffer: a frozen convolution skips its weight gradient (``resnet_backward``)
    no_buffer=lambda names, needs, c, plan: {n for n, nd in zip(names, needs) if not nd})
