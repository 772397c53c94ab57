"""LM-head loss without logits (``lm_head_stats``, ``lm_head_loss(fused=True)``, ``GPT.forward(fused_loss=True)``)
against fp64 from the same bf16 inputs: ``x = h.double() @ w[:V].double().T``, then the documented row formula.

Per-row bound for ``lse`` and ``xt``::

    tol_i = 2 * C * 2^-24 * A_i + 1e-5 * (1 + |lse_i|),      A_i = max_v sum_k |h_ik w_vk|   (fp64)

the worst case of an fp32 accumulation of C exact bf16 products in any order, plus slack for ``v_exp_f32``, ``log``
and the order of the vocabulary sum; for ``sx``: ``V * 2^-23 * mean_v |x_v| + C * 2^-23 * A_i``; for a loss row:
``tol_i * (1 + eps + 2 zc |lse_i|) * |w_i|``.  Each test prints its figures (``-s`` shows them).

Rows of every case (where N has them): 0 ordinary with its target in the last, ragged vocabulary tile; 1 scaled so
that ``|x|`` reaches 60; 2 with its maximum planted in the last tile and its target in the first slice; 3 both: a
maximum of about 60 that arrives last, so the running max grows late and rescales."""
import functools

import pytest
import torch

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import transformer as TR

pytestmark = pytest.mark.gpu

dev = "cuda"
CASES = [(1, 64, 8, 8), (130, 128, 257, 264), (257, 768, 50257, 50304)]   # N, C, V, Vp
IDS = ["one_tile", "ragged", "gpt2_vocab"]
EPS, ZC = 0.1, 1e-4


@functools.lru_cache(maxsize=None)
def _case(N, C, V, Vp):
    """bf16 h, w (pad rows zero), targets and the fp64 reference, computed once per shape and never changed."""
    g = torch.Generator().manual_seed(5)
    h = torch.randn(N, C, generator=g)
    w = torch.randn(Vp, C, generator=g) / C ** 0.5
    tg = torch.randint(0, V, (N,), generator=g)
    tg[0] = V - 1
    if N > 3:
        h[2] = 8 * w[V - 1]
        h[3] = w[V - 2]
        for i in (1, 3):
            h[i] *= 60 / (h[i] @ w[:V].T).abs().max()
        tg[2], tg[3] = 0, V - 2
    h, w = h.to(dev, torch.bfloat16), w.to(dev, torch.bfloat16)
    w[V:] = 0
    hd, wd, tg = h.double(), w[:V].double(), tg.to(dev)
    x = hd @ wd.T
    A = (hd.abs() @ wd.abs().T).max(1).values
    lse = torch.logsumexp(x, 1)
    ref = dict(lse=lse, xt=x.gather(1, tg[:, None])[:, 0], sx=x.sum(1), A=A)
    ref["tol"] = 2 * C * 2.0 ** -24 * A + 1e-5 * (1 + lse.abs())
    ref["tol_sx"] = V * 2.0 ** -23 * x.abs().mean(1) + C * 2.0 ** -23 * A
    return h, w, tg, ref


def _rows64(ref, tg, V, eps=0.0, zc=0.0, wts=None):
    """(fp64 loss rows, their tolerance) of the documented formula; rows with a negative target are 0."""
    wt = torch.ones_like(ref["lse"]) if wts is None else wts.double()
    valid = tg >= 0
    rows = wt * (ref["lse"] - (1 - eps) * ref["xt"] - eps / V * ref["sx"] + zc * ref["lse"] ** 2)
    tol = ref["tol"] * (1 + eps + 2 * zc * ref["lse"].abs()) * wt.abs()
    zero = rows.new_zeros(())
    return torch.where(valid, rows, zero), torch.where(valid, tol, zero)


@pytest.mark.parametrize("pad", [float("nan"), 1e4], ids=["pad_nan", "pad_1e4"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stats_against_fp64(case, pad):
    h, w, tg, ref = _case(*case)
    w = w.clone()
    w[case[2]:] = pad
    lse, xt, sx = TR.lm_head_stats(h, w, tg, case[2], with_sum=True)
    r = [((got.double() - ref[k]).abs() / ref[t]).max().item()
         for got, k, t in ((lse, "lse", "tol"), (xt, "xt", "tol"), (sx, "sx", "tol_sx"))]
    print(f"lm_head_stats {case}: max err/tol lse {r[0]:.4f} xt {r[1]:.4f} sx {r[2]:.4f}")
    assert max(r) <= 1.0
    assert TR.lm_head_stats(h, w, tg, case[2])[0].equal(lse)      # the instantiation without the row sum


def _flavour(name, N, tg):
    g = torch.Generator().manual_seed(9)
    if name == "plain":
        return {}, tg, None
    mask = torch.rand(N, generator=g).to(dev) < 0.7
    mask[:4] = True
    t2 = tg.clone()
    if N > 5:
        t2[5] = -100
    eff = torch.where(mask & (t2 != -100), t2, torch.full_like(t2, -1))
    kw = dict(ignore_index=-100, loss_mask=mask)
    if name == "smooth":
        wts = (2 * torch.rand(N, generator=g)).to(dev)
        return dict(kw, label_smoothing=EPS, z_loss=ZC, loss_weights=wts), t2, (eff, wts)
    return kw, t2, (eff, None)


@pytest.mark.parametrize("name", ["plain", "masked", "smooth", "denom"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_loss_flavours_against_fp64(case, name):
    (N, C, V, Vp), (h, w, tg, ref) = case, _case(*case)
    kw, t_in, m = _flavour(name, N, tg)
    eff, wts = (tg, None) if m is None else m
    smooth = name == "smooth"
    rows, tol = _rows64(ref, eff, V, EPS if smooth else 0.0, ZC if smooth else 0.0, wts)
    count = N if name == "plain" else max(int((eff >= 0).sum()), 1)
    with torch.no_grad():
        for red in ("mean",) if name == "denom" else ("none", "sum", "mean"):
            extra = dict(denom=torch.tensor(7.0, device=dev)) if name == "denom" else {}
            got = TR.lm_head_loss(h, w, t_in, V, reduction=red, fused=True, **kw, **extra).double()
            div = 7.0 if name == "denom" else count if red == "mean" else 1.0
            want, bound = (rows, tol) if red == "none" else (rows.sum() / div, tol.sum() / div)
            err = (got - want).abs()
            print(f"fused {name}/{red} {case}: max err {err.max().item():.3e}, bound there "
                  f"{bound.reshape(-1)[err.reshape(-1).argmax()].item():.3e}")
            assert (err <= bound).all()
            if red == "none":
                assert (got[eff < 0] == 0).all()


@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_invalid_rows_and_empty_batch(case):
    (N, C, V, Vp), (h, w, tg, ref) = case, _case(*case)
    tg = tg.clone()
    tg[[1, 7, N - 1]] = -1
    wts = torch.rand(N, device=dev) + 0.5
    kw = dict(ignore_index=-1, reduction="none", label_smoothing=EPS, fused=True)
    hp, wp = h.clone(), wts.clone()
    hp[1], hp[7], hp[N - 1] = float("nan"), float("inf"), -float("inf")
    wp[[1, 7, N - 1]] = float("nan")
    with torch.no_grad():
        clean = TR.lm_head_loss(h, w, tg, V, loss_weights=wts, **kw)
        dirty = TR.lm_head_loss(hp, w, tg, V, loss_weights=wp, **kw)
        none = torch.full_like(tg, -1)
        empty = TR.lm_head_loss(hp, w, none, V, ignore_index=-1, fused=True)
        empty_rows = TR.lm_head_loss(hp, w, none, V, loss_weights=wp, **kw)
    assert dirty.equal(clean) and (dirty[[1, 7, N - 1]] == 0).all() and (clean[tg >= 0] != 0).all()
    assert empty.item() == 0.0 and (empty_rows == 0).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_worse_than_logits_path(case):
    (N, C, V, Vp), (h, w, tg, ref) = case, _case(*case)
    rows = _rows64(ref, tg, V)[0]
    with torch.no_grad():
        old = (TR.lm_head_loss(h, w, tg, V, ignore_index=-1, reduction="none").double() - rows).abs()
        new = (TR.lm_head_loss(h, w, tg, V, ignore_index=-1, reduction="none", fused=True).double() - rows).abs()
    print(f"{case}: max row error fused {new.max().item():.3e}, through bf16 logits {old.max().item():.3e}")
    assert (new <= old).all()


@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_determinism_and_graph_replay(case):
    (N, C, V, Vp), (h, w, tg, ref) = case, _case(*case)
    h, tg, wts = h.clone(), tg.clone(), torch.ones(N, device=dev)
    kw = dict(ignore_index=-1, label_smoothing=EPS, z_loss=ZC, loss_weights=wts, fused=True)

    def run():
        return (TR.lm_head_loss(h, w, tg, V, reduction="none", **kw), TR.lm_head_loss(h, w, tg, V, **kw))

    with torch.no_grad():
        a, b = run(), run()
        assert a[0].equal(b[0]) and a[1].equal(b[1])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        for seed in (1, 2):
            g = torch.Generator(device=dev).manual_seed(seed)
            h.copy_(torch.randn(N, C, device=dev, generator=g))
            tg.copy_(torch.randint(-1, V, (N,), device=dev, generator=g))
            wts.copy_(torch.rand(N, device=dev, generator=g))
            graph.replay()
            eager = run()
            assert out[0].equal(eager[0]) and out[1].equal(eager[1]) and not out[0].equal(a[0])


def test_model_fused_loss(monkeypatch):
    cfg = GPTConfig(block_size=128, vocab_size=257, padded_vocab=264, n_layer=2, n_head=2, n_embd=128)
    model = build_gpt2(cfg, seed=0, device=dev)
    g = torch.Generator().manual_seed(3)
    idx, tg = (torch.randint(0, 257, (2, 128), generator=g).to(dev) for _ in range(2))
    seen, op = [], TR.lm_head_loss
    monkeypatch.setattr(TR, "lm_head_loss", lambda x, *a, **k: (seen.append(x), op(x, *a, **k))[1])
    with torch.no_grad():
        loss = model(idx, tg, fused_loss=True)
    hd, wd = seen[0].reshape(-1, 128).double(), model.transformer.wte.weight[:257].double()
    x = hd @ wd.T
    lse = torch.logsumexp(x, 1)
    want = (lse - x.gather(1, tg.reshape(-1, 1))[:, 0]).mean()
    tol = (2 * 128 * 2.0 ** -24 * (hd.abs() @ wd.abs().T).max(1).values + 1e-5 * (1 + lse.abs())).mean()
    print(f"model: fused {loss.item():.6f}, fp64 {want.item():.6f}, bound {tol.item():.2e}")
    assert abs(loss.item() - want.item()) <= tol.item()
    with pytest.raises(NotImplementedError, match="fused"):
        model(idx, tg, fused_loss=True)
