"""CPU: the host side of synchronised BatchNorm for the ResNet item tower -- the ``--sync_bn`` argument check, what
``torch.nn.SyncBatchNorm.convert_sync_batchnorm`` keeps (keys, parameter order, ``requires_grad``), the refusal of a half-converted
tower, the new exports, the rank-merge and rank-fold helpers of ``resnet_engine`` over two gloo ranks on host tensors, and the size of
the effect the GPU file's negative control relies on (per-rank statistics are another model)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import resnet_ref
from helpers import GOLDEN_DIR
from idvs.morec_amd import _lib, resnet_engine
from idvs.morec_amd.model.encoders import Resnet_Encoder
from idvs.morec_amd.model.resnet import HipResNet, ResNetShape
from idvs.morec_amd.parameters import check_resnet_args, parse_args
from idvs.morec_amd.utils.detgen import det_normal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g32_resnet_keys.json")))
SLAB = 1024      # rows per statistics partial (morec_bn_slab_rows(); the host partials below are cut the same way)
SPLITS = [(5, 131), (1, 1030)]


def test_sync_bn_flag_passes_the_argument_check(monkeypatch):
    base = ["--item_tower", "modal", "--CV_model_load", "resnet-50"]
    assert parse_args(base).sync_bn is False
    assert check_resnet_args(parse_args(base + ["--sync_bn"])) is True      # world size 1: accepted, does nothing
    assert check_resnet_args(parse_args(["--item_tower", "modal", "--CV_model_load", "swin_tiny", "--sync_bn"])) is False      # a no-op elsewhere
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert check_resnet_args(parse_args(base + ["--sync_bn"])) is True
    with pytest.raises(SystemExit, match="ResNet item tower.*SyncBatchNorm") as e:
        check_resnet_args(parse_args(base))
    assert "--sync_bn" in str(e.value)
    for extra, word in ((["--fused_step"], "--fused_step"), (["--graph"], "--graph"), (["--arch", "dssm"], "--arch dssm")):      # these stay
        with pytest.raises(SystemExit, match="ResNet item tower") as e:
            check_resnet_args(parse_args(base + ["--sync_bn"] + extra))
        assert word in str(e.value)


@pytest.mark.parametrize("name", ["resnet_micro", "resnet_micro_b"])
def test_conversion_keeps_keys_order_and_flags(name):
    enc = Resnet_Encoder(HipResNet(ResNetShape.named(name), 48), compute_dtype=torch.float32)
    for i, (_, p) in enumerate(enc.image_net.named_parameters()):      # --freeze_paras_before 5
        p.requires_grad = i >= 5
    sd0 = {k: v.clone() for k, v in enc.state_dict().items()}
    names0, flags0 = [n for n, _ in enc.named_parameters()], [p.requires_grad for p in enc.parameters()]
    ids0 = [id(p) for p in enc.parameters()]
    assert enc.sync_context() is None
    conv = torch.nn.SyncBatchNorm.convert_sync_batchnorm(enc)
    assert conv is enc and isinstance(enc.image_net, HipResNet) and enc.image_net.shape == ResNetShape.named(name)
    bns = [m for m in enc.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert bns and all(isinstance(m, torch.nn.SyncBatchNorm) for m in bns)
    assert list(enc.state_dict()) == list(sd0) and all(torch.equal(v, sd0[k]) for k, v in enc.state_dict().items())
    assert [n for n, _ in enc.named_parameters()] == names0 and [p.requires_grad for p in enc.parameters()] == flags0
    assert [id(p) for p in enc.parameters()] == ids0      # the same parameter objects: an optimizer built before the conversion still holds them
    assert [k for k, _ in enc.image_net.named_parameters()][:-2] == KEYS[name]["named_parameters"][:-2]
    assert [k for k in enc.image_net.state_dict()] == [k for k, _ in KEYS[name]["state_dict"]]
    assert enc.sync_context() is None      # no initialised process group: the plain path, as torch falls back


def test_mixed_batchnorm_and_syncbatchnorm_raises():
    enc = Resnet_Encoder(HipResNet(ResNetShape.named("resnet_micro"), 48), compute_dtype=torch.float32)
    enc.image_net.layer2 = torch.nn.SyncBatchNorm.convert_sync_batchnorm(enc.image_net.layer2)
    with pytest.raises(NotImplementedError, match="mixture of SyncBatchNorm.*layer2.*BatchNorm2d"):
        enc.sync_context()
    with pytest.raises(NotImplementedError, match="mixture"):      # before anything touches a device, in either mode
        enc.eval().encode(torch.zeros(1, 3, 32, 32))


def test_syncbn_exports_have_signatures():
    for n in ("morec_bn_bwd_fold", "morec_bn_bwd_apply_n"):
        assert n in _lib.EXPORTS and hasattr(_lib.lib(), n)
    assert len(_lib.lib().morec_bn_bwd_apply_n.argtypes) == len(_lib.lib().morec_bn_bwd_apply.argtypes) + 1      # the count pointer
    assert len(_lib.lib().morec_bn_bwd_fold.argtypes) == 5
    # refusals need no device: null pointers
    assert _lib.lib().morec_bn_bwd_fold(None, 2, 32, None, None) == -1
    assert _lib.lib().morec_bn_bwd_apply_n(None, None, None, None, None, None, None, None, None, None, 4, 32, _lib.F32, None) == -1
    header = open(os.path.join(ROOT, "include", "morec_hip.h")).read()
    assert "int morec_bn_bwd_fold(" in header and "int morec_bn_bwd_apply_n(" in header


def _host_partials(x):
    """fp32 [slabs, 3, C] the kernel's way: per slab of ``SLAB`` rows the count, the slab mean, the squares of the deviations from it."""
    out = []
    for r0 in range(0, x.shape[0], SLAB):
        s = x[r0:r0 + SLAB]
        m = s.mean(0)
        out.append(torch.stack([torch.full_like(m, float(s.shape[0])), m, ((s - m) ** 2).sum(0)]))
    return torch.stack(out)


def _case(split):
    g = torch.Generator().manual_seed(1000 * split[0] + split[1])
    x = (100.0 + torch.randn((sum(split), 16), generator=g, dtype=torch.float64)).float()
    sums = [torch.randn((2, 16), generator=g) * 50.0 for _ in split]
    return x, sums


def _worker(rank, world, port, q):
    import sys
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from syncbn_spawn import report

    def body():
        import datetime
        from idvs.morec_amd import resnet_engine as re_
        sync = re_.BnSync(None, world)      # (before the group exists: a tree without the feature fails here, at once)
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        out = []
        for split in SPLITS:
            x, sums = _case(split)
            r0 = sum(split[:rank])
            local = re_.merge_bn_partials(_host_partials(x[r0:r0 + split[rank]]))
            out.append((re_.merge_bn_over_ranks(local, sync).numpy(), re_.fold_bn_sums_over_ranks(sums[rank], sync).numpy()))
        return out

    report(q, rank, body)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_rank_merge_and_fold_two_gloo_ranks_on_host_tensors():
    """Mean-100 rows cut 5 / 131 and 1 / 1030 between two ranks: both ranks get the same bits; the merged mean and variance lie within
    ``test_merge_on_device_is_the_host_merge``'s fp64 bounds of the whole (|mean error| <= 80 x 2^-24 x 100, |M2 / n - var| < 1e-5); the
    folded sums are the fp64 total within one rounding per addition (W - 1 additions of values whose partial sums are bounded by the sum
    of magnitudes)."""
    from syncbn_spawn import run_ranks
    for helper in ("BnSync", "merge_bn_over_ranks", "fold_bn_sums_over_ranks"):      # nothing to spawn for without them
        assert hasattr(resnet_engine, helper), f"resnet_engine.{helper} is missing"
    got = run_ranks(_worker, 2, 30100 + os.getpid() % 200, timeout=200.0)
    for i, split in enumerate(SPLITS):
        (m0, f0), (m1, f1) = got[0][i], got[1][i]
        assert np.array_equal(m0, m1) and np.array_equal(f0, f1), split
        x, sums = _case(split)
        ref = x.double()
        assert (m0[0] == float(sum(split))).all()
        assert np.abs(m0[1].astype(np.float64) - ref.mean(0).numpy()).max() <= 80 * 2.0 ** -24 * 100
        assert np.abs(m0[2].astype(np.float64) / sum(split) - ref.var(0, unbiased=False).numpy()).max() < 1e-5
        # the merge over ranks is merge_bn_partials over the stacked rank results, in rank order
        locals_ = [resnet_engine.merge_bn_partials(_host_partials(x[sum(split[:r]):sum(split[:r + 1])])) for r in range(2)]
        assert np.array_equal(resnet_engine.merge_bn_partials(torch.stack(locals_)).numpy(), m0)
        tot64 = sum(s.double() for s in sums).numpy()
        mag = sum(s.double().abs() for s in sums).numpy()
        assert (np.abs(f0.astype(np.float64) - tot64) <= (len(split) - 1) * 2.0 ** -24 * mag).all()


@pytest.mark.parametrize("name", ["resnet_micro", "resnet_micro_b"])
def test_per_rank_statistics_are_another_model(name):
    """What the GPU file's negative control relies on, in fp64 on the plain-torch net: training-mode item vectors of the six golden images
    in one batch against the same images as two batches of three.  The whole reproduces g32; the split misses the fp32 bound of
    ``test_g32_encoder_golden`` (4 x the reference's own fp32 error) by orders of magnitude."""
    G = np.load(os.path.join(GOLDEN_DIR, "g32_resnet.npz"))
    n, R0, D = (int(v) for v in G["cfg"])
    x = det_normal("g32.x", (n, 3, R0, R0), std=1.0)
    x[0] = 0.0
    x = torch.from_numpy(x).double()
    ref64 = G[f"{name}.y64"]
    bound = 4.0 * float(np.abs(G[f"{name}.y"].astype(np.float64) - ref64).max())

    def run(shards):
        net = resnet_ref.load_det(resnet_ref.build(name, D), prefix="cv_encoder.image_net.").double().train()
        with torch.no_grad():
            return torch.cat([torch.nn.functional.gelu(net(s)) for s in shards]).numpy()

    whole, split = run([x]), run([x[:3], x[3:]])
    assert np.abs(whole - ref64).max() <= 1e-9
    err = float(np.abs(split - ref64).max())
    print(f"{name}: per-rank statistics (3 + 3) move y by {err:.3e}; the fp32 bound is {bound:.3e}")
    assert err > 100 * bound
