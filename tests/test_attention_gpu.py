"""The flash-attention kernels (``csrc/kernels/attention.hip``) and the decode attention
(``csrc/kernels/decode.hip``) against the fp64 reference of ``tests/attention_ref.py``, under its per-row
metric: structured score families, the LSE and ``D`` directly, every instantiation behind
``attn_set_variant`` and ``p > 0``, both row-stride layouts, and decode positions on both sides of every
chunk boundary.  ``BOUND`` is the measured noise floor of a bf16 emulation times 3 (test_attention_cpu.py);
the decode bound is derived.  Each test prints its worst errors (``-s`` shows them)."""
import functools
from types import SimpleNamespace

import pytest
import torch

from pytorch_distributed_example_amd._ext import kernels
from pytorch_distributed_example_amd.ops import DeviceRNG
from pytorch_distributed_example_amd.ops import decode as D
from pytorch_distributed_example_amd.ops import rng as R
from pytorch_distributed_example_amd.ops import transformer as TR

import attention_ref as A

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
OUTS = ("y", "dq", "dk", "dv")
ALL = OUTS + ("lse2", "D")

# (B, T, H): one query block and two key tiles; batch and head offsets; a tile count that is no power of
# two with a partial last head group in the block map; sixteen key tiles (the ring wraps five times)
SHAPES = [(1, 128, 1), (2, 256, 3), (3, 384, 5), (1, 1024, 2)]
STRUCT_SHAPES = [(2, 256, 3), (1, 1024, 2)]
CASES = [("gauss1", s) for s in SHAPES] + [(f, s) for f in A.FAMILIES if f != "gauss1" for s in STRUCT_SHAPES]


def _id(case):
    f, (B, T, H) = case
    return f"{f}-{B}x{T}x{H}"


@functools.lru_cache(maxsize=4)
def _inputs(family, B, T, H):
    """bf16 q, k, v, dO as [B, H, T, 64] on the CPU, built once per parameter set and never modified."""
    return A.make(family, B, H, T)


def _btc(t):
    B, H, T, _ = t.shape
    return t.transpose(1, 2).reshape(B, T, H * 64)


def _bhtd(t, H):
    B, T, _ = t.shape
    return t.reshape(B, T, H, 64).transpose(1, 2)


def _run(q, k, v, dO, layout="fused", drop=None):
    """``attn_fwd`` + ``attn_bwd`` called directly (the arguments of ``ops.transformer.CausalAttentionFn``),
    which makes ``lse`` and ``Dd`` visible.  ``layout``: "fused" (q/k/v are column blocks of one [B, T, 3C]
    buffer, row stride 3C), "split" (three contiguous buffers, row stride C) or "padded" (fused q/k/v, o and
    dO with a row stride of C + 64).  Every output buffer starts as NaN.  Returns CPU tensors, [B, H, T, ...]."""
    B, H, T, _ = q.shape
    C = 64 * H
    K = kernels()
    if layout == "split":
        qs, ks, vs = (_btc(t).contiguous().to(dev) for t in (q, k, v))
        dqs, dks, dvs = (torch.full_like(qs, NAN) for _ in range(3))
    else:
        qkv = torch.cat([_btc(q), _btc(k), _btc(v)], 2).to(dev)
        dqkv = torch.full_like(qkv, NAN)
        qs, ks, vs = (qkv[:, :, i * C:(i + 1) * C] for i in range(3))
        dqs, dks, dvs = (dqkv[:, :, i * C:(i + 1) * C] for i in range(3))
    if layout == "padded":
        obuf = torch.full((B, T, C + 64), NAN, device=dev, dtype=BF16)
        gbuf = torch.full((B, T, C + 64), NAN, device=dev, dtype=BF16)
        o, g = obuf[:, :, :C], gbuf[:, :, :C]
        g.copy_(_btc(dO))
    else:
        o = torch.full((B, T, C), NAN, device=dev, dtype=BF16)
        g = _btc(dO).contiguous().to(dev)
    lse = torch.full((B * H * T,), NAN, device=dev, dtype=torch.float32)
    Dd = torch.full((B * H * T,), NAN, device=dev, dtype=torch.float32)
    extra = () if drop is None else drop
    K.attn_fwd(qs, ks, vs, o, lse, H, A.SCALE, *extra)
    K.attn_bwd(qs, ks, vs, o, g, lse, Dd, dqs, dks, dvs, H, A.SCALE, *extra)
    torch.cuda.synchronize()
    if layout == "padded":                   # nothing was written between the rows
        assert obuf[:, :, C:].isnan().all()
    return SimpleNamespace(y=_bhtd(o.cpu(), H), dq=_bhtd(dqs.cpu(), H), dk=_bhtd(dks.cpu(), H), dv=_bhtd(dvs.cpu(), H),
                           lse2=lse.cpu().view(B, H, T), D=Dd.cpu().view(B, H, T))


def _same_bits(a, b):
    return [n for n in ALL if not torch.equal(getattr(a, n), getattr(b, n))]


def _where(name, idx):
    b, h, row = idx
    if name in ("y", "dq"):      # k_attn_fwd / k_attn_bwd_dq: query block row / 128, wave (row % 128) / 32
        return f"(b {b}, h {h}, query {row}: block {row // 128}, wave {row % 128 // 32}, last key tile {row // 64})"
    return f"(b {b}, h {h}, key {row}: block {row // 128}, wave {row % 128 // 32})"


def _check(got, q, k, v, dO, tag, **kw):
    """Every output of a kernel run against the reference.  The reference backward takes the kernels' own
    bf16 ``y`` for ``D = rowsum(dO * y)``, not the fp64 ``y``: that is the function ``k_attn_bwd_dq``
    implements (it is handed O, not the probabilities), and on rows where ``dO . y`` cancels the two differ by
    more than any rounding of the backward itself."""
    ref = A.reference(q, k, v, dO, y_for_D=got.y, **kw)
    fails, line = [], []
    for n in OUTS:
        e, idx = A.worst_row(getattr(got, n), getattr(ref, n), getattr(ref, "den_" + n))
        line.append(f"{n} {e:.5f}")
        if not e <= A.BOUND:
            fails.append(f"{n}: {e:.5f} > {A.BOUND:.5f} at {_where(n, idx)}")
    lse_e = ((got.lse2.double() - ref.lse2).abs() / ref.lse2.abs().clamp_min(1.0)).max().item()
    d_e = A.row_error(got.D.unsqueeze(-1), ref.D.unsqueeze(-1), ref.den_D.unsqueeze(-1))
    line += [f"lse2 {lse_e:.2e}", f"D {d_e:.2e}"]
    print(f"ATTN {tag}: " + " ".join(line))
    if not lse_e <= 1e-4:
        fails.append(f"lse2: {lse_e:.3e} > 1e-4")
    if not d_e <= 2.0 ** -8:
        fails.append(f"D: {d_e:.3e} > 2^-8")
    assert not fails, (tag, fails)
    return ref


@functools.lru_cache(maxsize=None)
def _default_run(family, B, T, H):
    """The default instantiations (variant 5) without dropout on the fused layout."""
    return _run(*_inputs(family, B, T, H))


# --------------------------------------------------------------------------------------- forward + backward
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_attention_against_fp64_reference(case):
    family, (B, T, H) = case
    q, k, v, dO = _inputs(family, B, T, H)
    if family == "leak":
        # the construction is potent: admitting the masked keys moves every query row but the last (which
        # has no key q + 1) by more than its whole magnitude
        masked = A.reference(q, k, v, dO)
        unmasked = A.reference(q, k, v, dO, allowed=torch.ones(T, T, dtype=torch.bool))
        moved = A.row_errors(unmasked.y, masked.y, masked.den_y)[..., :-1]
        assert moved.min().item() > 1.0, moved.min().item()
    got = _default_run(family, B, T, H)
    for n in ALL:
        assert torch.isfinite(getattr(got, n)).all(), (family, n)
    ref = _check(got, q, k, v, dO, _id(case))
    if family == "uniform":
        # q == 0: every row's key count is pinned (adjacent rows differ by 1.4e-3 at t = 1023)
        want = torch.log2(torch.arange(1, T + 1, dtype=torch.float64)).expand(B, H, T)
        e = (got.lse2.double() - want).abs().max().item()
        assert e <= 2e-5, e
    if family == "needle0":
        # the diagonal carries the whole weight: y is v, bit for bit
        sel = ref.P.diagonal(dim1=-2, dim2=-1) >= 1 - 2.0 ** -10
        assert sel.all()                                  # by construction (a peak of e^40 on the query's own key)
        assert torch.equal(got.y[sel], v[sel])


def test_attention_through_the_op_and_autograd():
    """``ops.transformer.causal_attention`` on the fused [B, T, 3C] layout wires the same kernels."""
    family, (B, T, H) = "leak", (2, 256, 3)
    q, k, v, dO = _inputs(family, B, T, H)
    qkv = torch.cat([_btc(q), _btc(k), _btc(v)], 2).to(dev).requires_grad_()
    y = TR.causal_attention(qkv, H)
    y.backward(_btc(dO).contiguous().to(dev))
    dq, dk, dv = (_bhtd(t, H) for t in qkv.grad.cpu().split(64 * H, dim=2))
    direct = _default_run(family, B, T, H)
    got = SimpleNamespace(y=_bhtd(y.detach().cpu(), H), dq=dq, dk=dk, dv=dv, lse2=direct.lse2, D=direct.D)
    _check(got, q, k, v, dO, "op-" + _id((family, (B, T, H))))
    assert not _same_bits(got, direct)


@pytest.mark.parametrize("family", ["gauss1", "needle63"])
def test_attention_layouts_agree_bit_for_bit(family):
    B, T, H = 2, 256, 3
    fused = _default_run(family, B, T, H)
    for layout in ("split", "padded"):
        other = _run(*_inputs(family, B, T, H), layout=layout)
        assert not _same_bits(other, fused), (layout, _same_bits(other, fused))


# --------------------------------------------------------------------------------------- instantiations
@pytest.mark.parametrize("family", ["gauss1", "incr"])
@pytest.mark.parametrize("shape", [(3, 384, 5), (1, 1024, 2)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", [0, 2, 7])
def test_attention_variants(variant, shape, family):
    """Variant 0: forward <4, 2> and dK/dV <4, 2>; 2: dQ <3, 3>; 7: all three on the 3-deep side (the default
    5 is forward <3, 3>, dQ <4, 2>, dK/dV <3, 2>).  Ring depth and occupancy change no arithmetic."""
    B, T, H = shape
    q, k, v, dO = _inputs(family, B, T, H)
    base = _default_run(family, B, T, H)
    try:
        kernels().attn_set_variant(variant)
        got = _run(q, k, v, dO)
    finally:
        kernels().attn_set_variant(5)
    _check(got, q, k, v, dO, f"variant{variant}-" + _id((family, shape)))
    assert not _same_bits(got, base), _same_bits(got, base)


@pytest.mark.parametrize("family", ["gauss1", "incr", "leak"])
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_dropout(p, shape, family):
    B, T, H = shape
    site = 3
    q, k, v, dO = _inputs(family, B, T, H)
    seed = 100 + int(p * 10)
    snap_gpu, snap_cpu = DeviceRNG(seed, device=dev).next(), DeviceRNG(seed).next()
    assert R.snapshot_words(snap_gpu) == R.snapshot_words(snap_cpu)
    mask = R.dropout_mask(snap_cpu, site, p, bht=(B, H, T))
    keep = 1.0 - R.effective_p(p, "attention")
    assert abs(mask.double().mean().item() - keep) < 0.01              # it does drop, and about p of them
    got = _run(q, k, v, dO, drop=(snap_gpu, site, R.threshold(p, "attention"), 1.0 / keep))
    _check(got, q, k, v, dO, f"drop{p}-" + _id((family, shape)), mask=mask, inv_keep=1.0 / keep)
    # the LSE is undropped by design: the p = 0 run's, bit for bit
    assert torch.equal(got.lse2, _default_run(family, B, T, H).lse2)


# --------------------------------------------------------------------------------------- decode attention
class _Cfg:
    n_layer, n_head, n_embd = 1, 2, 128


DEC_H, DEC_TMAX = 2, 512
DEC_POS = (0, 1, 126, 127, 128, 129, 255, 256, 383, 384, 511)      # both sides of every 128-key chunk edge
DEC_FAMILIES = ("randn", "needle_chunk0", "needle_chunk1", "needle_chunk2", "needle_chunk3", "needle_new",
                "incr", "decr", "uniform")


@functools.lru_cache(maxsize=None)
def _dec_sequence(family, B):
    """K and V rows of positions 0 .. 511, [B, H, 512, 64] bf16 on the CPU: row p is the new token's at
    position p, the rows before it are the cache."""
    g = torch.Generator().manual_seed(len(family) * 31 + B)
    Ks = torch.randn(B, DEC_H, DEC_TMAX, 64, generator=g, dtype=torch.float64)
    Vs = torch.randn(B, DEC_H, DEC_TMAX, 64, generator=g, dtype=torch.float64)
    if family.startswith("needle"):
        Ks = A.PEAK * Ks / Ks.norm(dim=-1, keepdim=True)
    if family in ("incr", "decr"):
        t = (torch.arange(DEC_TMAX, dtype=torch.float64) / 16).to(BF16).double()
        Ks[..., 63] = t if family == "incr" else -t
    if family == "uniform":
        Vs = torch.randint(-8, 9, Vs.shape, generator=g).double()
    return Ks.to(BF16), Vs.to(BF16)


def _dec_query(family, B, p, Ks):
    """The query at position p, [B, H, 64] bf16; ``None`` where the family has no case at p."""
    g = torch.Generator().manual_seed(1000 + p)
    q = torch.randn(B, DEC_H, 64, generator=g, dtype=torch.float64)
    if family.startswith("needle_chunk"):
        j = 128 * int(family[-1]) + 37
        if j >= p:
            return None
        q = Ks[:, :, j].double()                  # score 40 at cache row j, about N(0, 5) elsewhere
    elif family == "needle_new":
        q = Ks[:, :, p].double()                  # the peak is the new key: it comes from the c_attn row
    elif family in ("incr", "decr"):
        q[..., 63] = 4.0                          # score +-t / 32: the chunk maxima are 4 apart
    elif family == "uniform":
        q = torch.zeros_like(q)
    return q.to(BF16)


def _dec_call(cache, q, Ks, Vs, positions, poison=False):
    """One ``decode_attention`` launch with row b at ``positions[b]``: the cache holds rows ``< p_b`` of the
    sequence, row ``p_b`` of the cache holds another token's K / V (the new ones must come from the c_attn
    row) and the rows past it random values, or 3e38 with ``poison``.  Returns ``[B, H, 64]`` on the CPU."""
    B = q.shape[0]
    Kc, Vc = Ks.clone(), Vs.clone()
    kn, vn = torch.empty_like(q), torch.empty_like(q)
    for b, p in enumerate(positions):
        kn[b], vn[b] = Ks[b, :, p], Vs[b, :, p]
        Kc[b, :, p], Vc[b, :, p] = Ks[b, :, (p + 1) % DEC_TMAX], Vs[b, :, (p + 1) % DEC_TMAX]
        if poison:
            Kc[b, :, p + 1:], Vc[b, :, p + 1:] = 3e38, 3e38
    cache.data[0, 0].copy_(Kc)
    cache.data[0, 1].copy_(Vc)
    base = max(positions)
    state = D.DecodeState(dev, pos=base, row_offsets=[p - base for p in positions])
    qkv = torch.cat([t.reshape(B, DEC_H * 64) for t in (q, kn, vn)], 1).to(dev)
    y = D.decode_attention(qkv, cache, 0, state).cpu().view(B, DEC_H, 64)
    for b, p in enumerate(positions):             # the new K / V landed in row p_b, bit for bit
        assert torch.equal(cache.data[0, 0, b, :, p].cpu(), kn[b]) and torch.equal(cache.data[0, 1, b, :, p].cpu(), vn[b])
    return y


def _dec_check(y, q, Ks, Vs, positions, tag):
    worst = 0.0
    for b, p in enumerate(positions):
        ref, den = A.decode_reference(q[b:b + 1], Ks[b:b + 1, :, :p + 1], Vs[b:b + 1, :, :p + 1])
        e = A.row_error(y[b:b + 1], ref, den)
        assert e <= A.DECODE_BOUND, (tag, b, p, e)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("family", DEC_FAMILIES)
@pytest.mark.parametrize("B", [1, 3])
def test_decode_attention_against_fp64_reference(B, family):
    cache = D.KVCache(_Cfg, B, DEC_TMAX, dev)
    Ks, Vs = _dec_sequence(family, B)
    worst, ran = 0.0, 0
    for p in DEC_POS:
        q = _dec_query(family, B, p, Ks)
        if q is None:
            continue
        y = _dec_call(cache, q, Ks, Vs, [p] * B)
        worst = max(worst, _dec_check(y, q, Ks, Vs, [p] * B, (family, p)))
        ran += 1
        if family == "uniform":
            # sums of small integers are exact in fp32 and the division is correctly rounded: where the mean
            # is a bf16 value the output is that value
            mean = Vs[:, :, :p + 1].double().mean(2)
            exact = mean.to(BF16).double() == mean
            assert torch.equal(y.double()[exact], mean[exact]), p
            assert exact.all() or p > 1                       # one or two keys: always representable
    assert ran
    print(f"DECODE {family} B={B}: worst {worst:.5f} over {ran} positions (bound {A.DECODE_BOUND:.5f})")


@pytest.mark.parametrize("B", [1, 3])
def test_decode_attention_never_reads_past_its_position(B):
    """Cache rows past p hold 3e38 in K and V (0 * 3e38 would still be finite, 3e38 * anything else is not):
    the kernel zero-fills them instead of loading them, so the output is the clean run's bit for bit."""
    cache = D.KVCache(_Cfg, B, DEC_TMAX, dev)
    Ks, Vs = _dec_sequence("randn", B)
    for p in DEC_POS:
        q = _dec_query("randn", B, p, Ks)
        clean = _dec_call(cache, q, Ks, Vs, [p] * B)
        dirty = _dec_call(cache, q, Ks, Vs, [p] * B, poison=True)
        assert torch.isfinite(dirty).all() and torch.equal(dirty, clean), p
        _dec_check(dirty, q, Ks, Vs, [p] * B, ("poison", p))


@pytest.mark.parametrize("family", ["randn", "needle_new", "incr"])
def test_decode_attention_ragged_rows(family):
    """Rows of one batch at positions 5, 128 and 300 in the same launch (``DecodeState`` row offsets)."""
    B, positions = 3, [5, 128, 300]
    cache = D.KVCache(_Cfg, B, DEC_TMAX, dev)
    Ks, Vs = _dec_sequence(family, B)
    q = torch.stack([_dec_query(family, B, p, Ks)[b] for b, p in enumerate(positions)])
    y = _dec_call(cache, q, Ks, Vs, positions)
    worst = _dec_check(y, q, Ks, Vs, positions, (family, "ragged"))
    print(f"DECODE ragged {family}: worst {worst:.5f}")
    for b, p in enumerate(positions):             # and each row is the uniform-position launch's, bit for bit
        assert torch.equal(_dec_call(cache, q, Ks, Vs, [p] * B)[b], y[b]), (b, p)
