"""Model-level parity beyond 256 positions: the recipe of ``test_oracle_midsize_all_grads`` (tests/test_model_gpu.py: every parameter
gradient of a mid-size modal model against the CPU oracle, the same model and the same bounds (5e-5, 5e-4) / (2e-3, 2e-2)) with behaviour
sequences of 260 items (SASRec beyond 256, left-padded users: every padded position is a query row without a kept key) and with titles of
264 tokens (BERT beyond 256, ``max_position_embeddings = 264``), on the streaming attention kernels (csrc/attention_stream.hip); and one
fused ``TrainStep`` at (260, 30) in fp16, packed and unpacked, against the module path's loss."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from idvs.morec_amd.model import BertShape, HipBertModel, Model  # noqa: E402
from test_model_gpu import DEV, load_det, make_args, relerr  # noqa: E402

D, ITEM_NUM = 128, 300
# Seed of the data: 11, the recipe's seed for its longer shapes.  S = 260 takes 12, for the reason the recipe gives for its own seed rule: with
# 11 the data puts ONE pre-activation of the SASRec FFN of block 1 within rounding of 0, where ReLU' of the GPU and of the CPU oracle
# legitimately disagree.  Measured in fp32: the gradient of w_1 of block 1 is off by 3.4e-3 of its maximum in 34 of its 65536 elements, all of
# them in row 40 (one hidden unit), with its bias and what lies below it following (position embedding 2.4e-3, w_1 of block 0 1.7e-4) and the
# loss exact to 1.9e-6; with seeds 12 and 13 the same model on the same kernels is at 2.1e-6 / 1.4e-6 in every parameter.
SEEDS = {260: 12}


def _build(S, T, B, dt, seed=None):
    shape = BertShape(vocab_size=2000, hidden_size=128, num_hidden_layers=3, num_attention_heads=4,
                      intermediate_size=512, max_position_embeddings=max(64, T))
    rng = np.random.default_rng(SEEDS.get(S, 11) if seed is None else seed)
    pop = rng.random(ITEM_NUM + 1) + 0.05
    pop[1:] /= pop[1:].sum()
    pop[0] = 1
    args = make_args(max_seq_len=S, embedding_dim=D, word_embedding_dim=128, compute_dtype=dt, num_words_title=T)
    m = load_det(Model(args, ITEM_NUM, True, HipBertModel(shape), pop)).to(DEV)
    m.eval()
    content = np.zeros((ITEM_NUM + 1, 2 * T), dtype=np.int64)
    for i in range(1, ITEM_NUM + 1):
        L = int(rng.integers(3, T + 1))
        content[i, :L] = rng.integers(1, 2000, L)
        content[i, T:T + L] = 1
    ids = np.zeros((B, S + 1), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(rng.integers(2, S + 2))      # left-padded users
        ids[b, S + 1 - L:] = rng.integers(1, ITEM_NUM + 1, L)
        lm[b, S + 1 - L:] = 1
    return args, shape, pop, m, ids, content[ids.reshape(-1)], lm


def measure(S, T, B, dt, seed=None):
    """(|loss - oracle loss|, {parameter: gradient error}, largest |gradient| where the oracle's is zero): fp32 element-wise relative to
    the largest reference element, 16-bit the error of the whole tensor (test_oracle_midsize_all_grads)."""
    import morec_oracle as orc
    args, shape, pop, m, ids, items, lm = _build(S, T, B, dt, seed)
    loss = m(torch.from_numpy(ids).to(DEV).view(-1), torch.from_numpy(items).to(DEV), torch.from_numpy(lm).to(DEV), DEV)
    gs = 256.0 if dt.startswith("fp16") else 1.0
    (loss * gs).backward()
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    ref = orc.model_forward(p, torch.from_numpy(ids).view(-1), torch.from_numpy(items), torch.from_numpy(lm), pop,
                            max_seq_len=S, embedding_dim=D, n_heads=2, use_modal=True, bert_heads=4)
    ref.backward()
    errs, zero = {}, 0.0
    for k, v in m.named_parameters():
        if "pooler" in k:
            continue
        gref = p[k].grad
        got = v.grad.float() / gs
        if gref.abs().max().item() < 1e-7:   # e.g. key biases: mathematically zero gradient
            zero = max(zero, got.abs().max().item())
        elif dt == "fp32":
            errs[k] = relerr(got.cpu().numpy(), gref.numpy())
        else:
            errs[k] = float((got.cpu().double() - gref.double()).norm() / gref.double().norm())
    return abs(loss.item() - ref.item()), errs, zero


# (loss, gradient) bounds: those of test_oracle_midsize_all_grads, unchanged.  Measured (loss, worst gradient), with the same quantity at 256
# positions on the default (row-strip) kernels of the same build and the same seed next to it:
#     (260, 30) fp32  0.0e+00, 2.1e-6   | (256, 30)  0.0e+00, 3.1e-6        (10, 264) fp32  4.8e-7, 4.0e-6   | (10, 256)  4.8e-7, 3.0e-6
#     (260, 30) fp16  5.3e-4,  9.8e-3   | (256, 30)  3.6e-4,  9.9e-3        (10, 264) fp16  6.7e-4, 7.2e-3   | (10, 256)  1.4e-3, 2.5e-2
BOUNDS = {"fp32": (5e-5, 5e-4), "fp16": (2e-3, 2e-2)}


@pytest.mark.parametrize("S,T,B,dt", [(260, 30, 4, "fp32"), (260, 30, 4, "fp16"), (10, 264, 6, "fp32"), (10, 264, 6, "fp16")])
def test_oracle_beyond_256_positions_all_grads(S, T, B, dt):
    e_loss, errs, zero = measure(S, T, B, dt)
    tol_l, tol_g = BOUNDS[dt]
    worst = max(errs, key=errs.get)
    print(f"({S}, {T}) {dt}: loss diff {e_loss:.2e} < {tol_l}; worst gradient error {errs[worst]:.2e} < {tol_g} ({worst}); "
          f"zero-gradient parameters {zero:.1e}")
    assert e_loss < tol_l
    assert zero < (1e-5 if dt == "fp32" else 1e-3)
    assert not {k: e for k, e in errs.items() if not e < tol_g}


def test_train_step_beyond_256_positions():
    """One fused step at (260, 30) in fp16, with the host-prepared unpadded token layout and without it: the module path's loss."""
    from idvs.morec_amd import engine
    from idvs.morec_amd.train_step import TrainStep
    S, T, B = 260, 30, 4
    args, shape, pop, m, ids, items, lm = _build(S, T, B, "fp16")
    ids_d, items_d, lm_d = torch.from_numpy(ids).to(DEV).view(-1), torch.from_numpy(items).to(DEV), torch.from_numpy(lm).to(DEV)
    with torch.no_grad():
        want = m(ids_d, items_d, lm_d, DEV).item()
    for packed in (False, True):
        m2 = load_det(Model(args, ITEM_NUM, True, HipBertModel(shape), pop)).to(DEV)
        m2.eval()
        ts = TrainStep(m2, lr=1e-4, fine_tune_lr=5e-5, l2_weight=0.0, fine_tune_l2_weight=0.0, pool_negatives=False, loss_scale=256.0)
        pack = None
        if packed:
            rows = items_d.cpu()      # one text attribute: one (cu_seqlens, tok_idx, order, inv) tuple
            pack = tuple(t.to(DEV) for t in engine.token_packing_host(rows[:, T:], rows[:, :T]))
        loss = ts.forward_backward(ids_d, items_d, lm_d, token_packing=pack)
        ts.reduce_gradients()
        torch.cuda.synchronize()
        print(f"fused step (260, 30) fp16 packed={packed}: loss {loss.item():.6f}, module path {want:.6f}")
        assert abs(loss.item() - want) < 5e-3, (packed, loss.item(), want)
