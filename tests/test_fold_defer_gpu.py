"""-m gpu: deferred folds of the deterministic mode (``morec_fold_defer_begin`` / ``morec_fold_flush`` / ``morec_fold_defer_end``).
Under a scope the fixed-order folds into parameter gradients are queued and launched later, as one batched kernel, on another stream.
Checked with ``torch.equal`` (the batched kernel reproduces the summation tree of the in-place launches, so there is no tolerance):
every producer at ragged sizes -- ``n_parts`` of 1, 15, 16, 17, 63, 64, 65, ~500, row counts that are no multiple of the row block,
N = 768 / 2304 / 3072 --, destinations that already hold values, two jobs queued onto the same destination; two steps of a small
``TrainStep`` with the knob on and off; and a second step that allocates nothing inside the library."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_PARTS = [1, 15, 16, 17, 63, 64, 65, 500]


def _rnd(*shape, dt=torch.float32, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).to(DEV)


def _check(run, sizes, repeat=1):
    """``run(dsts)`` issues producers that add into the fp32 vectors ``dsts`` (one per entry of ``sizes``), ``repeat`` times over (two jobs on
    the same destination).  In place, then under a scope with the flush on a second stream: the same bits.  Returns jobs queued."""
    from idvs.morec_amd import ops
    ops.set_deterministic(True)
    try:
        def fresh():
            return [torch.full((n,), 0.25 + 0.5 * i, device=DEV) for i, n in enumerate(sizes)]      # destinations that already hold values
        want = fresh()
        for _ in range(repeat):
            run(want)
        torch.cuda.synchronize()
        got = fresh()
        before = [t.clone() for t in got]
        jobs0 = ops.fold_stats()["jobs"]
        assert ops.fold_defer_begin(), "no scope opened in the deterministic mode"
        try:
            for _ in range(repeat):
                run(got)
            jobs = ops.fold_stats()["jobs"] - jobs0
            torch.cuda.synchronize()
            if jobs:      # nothing has been added yet: the gradient is defined only behind the flush
                assert all(torch.equal(a, b) for a, b in zip(got, before))
            side = torch.cuda.Stream()
            ops.stream_wait_stream(side.cuda_stream)
            ops.fold_flush(side.cuda_stream)
            torch.cuda.current_stream().wait_stream(side)
        finally:
            ops.fold_defer_end()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (i, float((a.double() - b.double()).abs().max()))
        for a, b in zip(want, before):
            assert not torch.equal(a, b)
        return jobs
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("repeat", [1, 2])
@pytest.mark.parametrize("n_parts", N_PARTS)
def test_layernorm_bwd_partials(n_parts, repeat):
    """ln_bwd (layernorm.hip): 16 rows per block up to 8192 rows, so M = 16 n_parts - 5 leaves n_parts partial rows, the last one ragged."""
    from idvs.morec_amd import ops
    M, N, dt = 16 * n_parts - 5, 768, torch.float16
    z, dy_a, dy_b = _rnd(M, N, dt=dt, seed=1), _rnd(M, N, dt=dt, seed=2), _rnd(M, N, dt=dt, seed=3)
    mean, rstd, gamma = _rnd(M, seed=4, scale=0.1), 1.0 + 0.1 * _rnd(M, seed=5).abs(), 1.0 + 0.1 * _rnd(N, seed=6)

    def run(d):
        ops.layernorm_bwd(dy_a, dy_b, z, mean, rstd, gamma, d[0], d[1], dbias=d[2])
    assert _check(run, [N, N, N], repeat) == 3 * repeat


@pytest.mark.parametrize("n_parts", [1, 17, 65, 500])
def test_layernorm_bwd_res32_partials(n_parts):
    """ln_bwd of the fp32 residual stream (layernorm_res32.hip)."""
    from idvs.morec_amd import ops
    M, N, dt = 16 * n_parts - 3, 768, torch.bfloat16
    z32, dy16, dy32 = _rnd(M, N, seed=1), _rnd(M, N, dt=dt, seed=2, scale=0.3), _rnd(M, N, seed=3, scale=0.3)
    mean, rstd, gamma = _rnd(M, seed=4, scale=0.1), 1.0 + 0.1 * _rnd(M, seed=5).abs(), 1.0 + 0.1 * _rnd(N, seed=6)

    def run(d):
        ops.layernorm_bwd(dy16, dy32, z32, mean, rstd, gamma, d[0], d[1], dbias=d[2])
    assert _check(run, [N, N, N]) == 3


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("M,N", [(300, 768), (512 * 15 + 7, 2304), (512 * 17 - 1, 3072), (512 * 64 + 1, 768)])
def test_colsum_typed(M, N, dt):
    """morec_colsum (gemm.hip): row blocks of 512, the last one ragged; a single row block goes through a partial row under a scope."""
    from idvs.morec_amd import ops
    x = _rnd(M, N, dt=dt, seed=M)
    assert _check(lambda d: ops.colsum_(x, d[0]), [N], repeat=2) == 2


@pytest.mark.parametrize("M,N,K", [(131, 3072, 768), (1000, 3072, 768), (4099, 3072, 768), (20011, 3072, 768), (2049, 768, 768),
                                   (24, 256, 64), (200, 256, 64)])
def test_gemm_colsum_epilogue(M, N, K):
    """colsum_f32_launch behind the activation-derivative GEMM (gemm8p.hip / gemm2w.hip / gemm_nt_generic.hpp): per-tile rows, summed and
    folded by ONE job that reads the library's scratch instead of the caller's workspace.  (M = 24: a partly filled tile still writes
    one partial row per wave row -- the scratch region is sized over whole tiles.)"""
    from idvs.morec_amd import ops
    from idvs.morec_amd._lib import DACT_MUL
    dt = torch.bfloat16
    a, b, u = _rnd(M, K, dt=dt, seed=1, scale=0.2), _rnd(N, K, dt=dt, seed=2, scale=0.2), _rnd(M, N, dt=dt, seed=3)
    outs = []

    def run(d):
        outs.append(ops.gemm_nt(a, b, dact=DACT_MUL, dact_in=u, colsum_out=d[0]))
    assert _check(run, [N], repeat=2) == 2
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


@pytest.mark.parametrize("n_seq", [3, 100, 1001])
def test_attention_dbias(n_seq):
    """morec_attn_bwd_dbias (attention.hip): one fp32 row per sequence, N = 2304."""
    from idvs.morec_amd import ops
    T, nh, dh, dt = 30, 12, 64, torch.bfloat16
    H = nh * dh
    qkv, dctx = _rnd(n_seq * T, 3 * H, dt=dt, seed=1, scale=0.7), _rnd(n_seq * T, H, dt=dt, seed=2)
    keep = torch.ones(n_seq, T, device=DEV)
    keep[::3, T - 7:] = 0
    desc = ops.attn_desc(n_seq, T, nh, dh, False, dh ** -0.5, ops.FLT_MIN_MASK, dt)
    assert _check(lambda d: ops.attn_bwd(desc, qkv, keep, dctx, dbias=d[0]), [3 * H], repeat=2) == 2


@pytest.mark.parametrize("n_seq", [5, 300, 2100])
def test_embedding_position_and_type_rows(n_seq):
    """pos_grad.hpp through morec_bert_embed_bwd (embed.hip): [seq blocks][T][H] partial rows for the positions, one row per block for the type."""
    from idvs.morec_amd import ops
    T, H, V, dt = 30, 768, 200, torch.float16
    g = torch.Generator(device="cpu").manual_seed(n_seq)
    ids = torch.randint(0, V, (n_seq * T,), generator=g).to(torch.int32)
    order = torch.argsort(ids, stable=True).to(torch.int32).to(DEV)
    ids = ids.to(DEV)
    dz = _rnd(n_seq * T, H, dt=dt, seed=1)
    words = []

    def run(d):
        dw = torch.zeros(V, H, device=DEV)
        ops.bert_embed_bwd_(ids, dz, dw, d[0].view(T + 2, H), d[1], 0, T, order)
        words.append(dw)
    assert _check(run, [(T + 2) * H, H]) == 2
    assert torch.equal(words[0], words[1])      # the word rows (their own in-place fold) take their partials from the scope's scratch too


def _steps(defer, steps=2, wgrad_stream=True, tower="text", B=24):
    import bench
    from idvs.morec_amd import _lib, engine, ops
    from idvs.morec_amd.model import BertShape, HipBertModel, Model
    from idvs.morec_amd.train_step import TrainStep
    S, T, D, item_num = 12, 30, 128, 1500
    ids_all = bench.synth_batches(steps, B, S, item_num, np.random.default_rng(2))
    for i in range(steps):
        ids_all[i][::3, :4] = 0
    counts = np.bincount(ids_all.reshape(-1), minlength=item_num + 1).astype(np.float64) + 1.0
    pop = counts / counts[1:].sum()
    pop[0] = 1.0
    ops.set_deterministic(True)
    _lib.lib().morec_tuning_set(b"fold_defer", int(defer))
    was = engine.WgradStream.enabled
    engine.WgradStream.enabled = wgrad_stream
    try:
        torch.manual_seed(7)
        if tower == "vision":      # Swin micro: plain + shifted windows, a patch merging (its bias tiles are read inside the backward: folded in place)
            from idvs.morec_amd.model.swin import HipSwinForImageClassification
            from idvs.morec_amd.swin_engine import SwinShape
            shape = SwinShape.named("swin_micro")
            gen = torch.Generator(device=DEV).manual_seed(11)
            catalog = torch.randn((item_num + 1, 3, shape.image_size, shape.image_size), device=DEV, generator=gen)
            catalog[0].zero_()
            args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                                         CV_model_load="swin_micro", compute_dtype="fp16")
            m = Model(args, item_num, True, HipSwinForImageClassification(shape, D), pop).to(DEV).train()
        else:
            content = bench.synth_catalog(item_num, T, np.random.default_rng(1))
            shape = BertShape.named("tiny")
            args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                                         num_words_title=T, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                         bert_model_load="bert_tiny", word_embedding_dim=shape.hidden_size, compute_dtype="fp16")
            m = Model(args, item_num, True, HipBertModel(shape, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), pop).to(DEV).train()
        ts = TrainStep(m, lr=3e-3, fine_tune_lr=1e-3, l2_weight=0.01, fine_tune_l2_weight=0.01, pool_negatives=False, loss_scale=1024.0)
        losses, stats = [], []
        for i in range(steps):
            ids = torch.from_numpy(ids_all[i]).to(DEV)
            lm = (ids[:, :-1] != 0).float()
            if tower == "vision":
                losses.append(ts.step(ids.view(-1), catalog[ids.view(-1)], lm))
            else:
                rows = content[ids_all[i].reshape(-1)]
                pack = tuple(t.to(DEV) for t in engine.token_packing_host(rows[:, T:], rows[:, :T]))
                losses.append(ts.step(ids.view(-1), torch.from_numpy(rows).to(DEV), lm, token_packing=pack))
            stats.append(ops.fold_stats())
        ts.flush()
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        state.update({f"arena{gi}.{n}": getattr(g["arena"], n).clone() for gi, g in enumerate(ts.groups) for n in ("grad", "exp_avg", "exp_avg_sq")})
        return [float(x) for x in losses], state, stats
    finally:
        engine.WgradStream.enabled = was
        _lib.lib().morec_tuning_set(b"fold_defer", 1)
        ops.set_deterministic(False)


@pytest.mark.parametrize("tower,wgrad_stream,B", [("text", True, 24), ("text", False, 24), ("vision", True, 24), ("text", True, 3)])
def test_train_step_same_bits_with_and_without_deferral(tower, wgrad_stream, B):
    """Two steps of a BERT-tiny text step (and of a Swin-micro one; B = 3: products smaller than one GEMM tile): every parameter, gradient
    and AdamW moment with the folds deferred equals the in-place run."""
    on = _steps(True, wgrad_stream=wgrad_stream, tower=tower, B=B)
    off = _steps(False, wgrad_stream=wgrad_stream, tower=tower, B=B)
    assert on[2][-1]["jobs"] > on[2][0]["jobs"] and off[2][-1]["jobs"] == off[2][0]["jobs"]      # the knob is what differs
    assert on[0] == off[0], (on[0], off[0])
    assert on[1].keys() == off[1].keys()
    for k in on[1]:
        assert torch.equal(on[1][k], off[1][k]), (k, float((on[1][k].double() - off[1][k].double()).abs().max()))


def test_second_step_allocates_nothing():
    """The scope's scratch is sized while the first step runs; a further step of the same shapes queues and flushes without a device allocation."""
    _steps(True, steps=1)      # (sizes the scratch if no earlier test has)
    _, _, stats = _steps(True, steps=3)
    assert stats[1]["jobs"] > stats[0]["jobs"] and stats[1]["launches"] > stats[0]["launches"]
    assert stats[2]["allocations"] == stats[1]["allocations"] == stats[0]["allocations"], stats
    assert stats[2]["scratch_bytes"] == stats[0]["scratch_bytes"] > 0
