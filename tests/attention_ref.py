"""fp64 reference, per-row metric, input families, bf16 emulation and mask mutations for the attention
tests (``test_attention_cpu.py`` / ``test_attention_gpu.py``).  Plain torch on the CPU, no autograd.

Everything here works on ``[B, H, T, 64]`` tensors; the inputs are the bf16 values a kernel sees, upcast
to fp64.  ``scale = 1 / 8`` (head dim 64) throughout.

* ``reference`` -- causal attention forward and backward written out: ``y``, the base-2 log-sum-exp of
  the scaled scores (what ``k_attn_fwd`` stores), ``D = rowsum(dO * y)``, ``dq``, ``dk``, ``dv``, and the
  metric's denominators.  With a dropout keep-mask it follows the header of ``csrc/kernels/attention.hip``.
* ``row_error`` -- the metric: per row ``||got - ref||_2 / ||den||_2`` with ``den`` the same contraction over
  absolute values (the magnitude before cancellation), maximum over all rows.
* the input families (``FAMILIES``), each a function of ``(B, H, T, seed)``.
* ``emulate`` -- the kernels' bf16 rounding points in fp64 arithmetic.  It measures the noise floor of the
  metric (``BOUND`` is three times that floor) and is never an expected value.
* ``mutate`` -- deliberately wrong causal masks, to show that the metric sees what ``max|a-b| / max|b|``
  does not.
"""
import math
from types import SimpleNamespace

import torch

HD = 64
SCALE = 1.0 / math.sqrt(HD)
LN2 = math.log(2.0)
BF16 = torch.bfloat16
F64 = torch.float64

# Three times the worst row error of `emulate` against `reference` over every family and output at
# T = 1024, with and without dropout (test_attention_cpu.py::test_floor_*; the figures are in
# profiles/attention_tests/README.md).  The factor 3 is for what the emulation does not model: MFMA
# accumulation order, fp32 partial sums, exp2 against exp.
FLOOR = 0.00455                     # measured: `big`, dv
BOUND = 3 * FLOOR                   # 0.01365

# Decode attention keeps fp32 probabilities: its one rounding is the bf16 output, within 2^-9 relative per
# element (round to nearest), so within 2^-9 of |y| <= P @ |V| per row; a factor 2 for the fp32 sums.
DECODE_BOUND = 2.0 ** -8


def causal_allowed(T):
    """bool [T(query), T(key)]: key <= query."""
    return torch.ones(T, T, dtype=torch.bool).tril()


def _up(*ts):
    return tuple(None if t is None else t.to(F64) for t in ts)


# ------------------------------------------------------------------------------------------ reference
def reference(q, k, v, dO, mask=None, inv_keep=1.0, y_for_D=None, allowed=None, v_src=None):
    """Causal attention and its gradients in fp64, written out.

    ``mask`` is a keep-mask ``[B, H, T, T]`` (``ops.rng.attention_mask``): the row sum ``l`` and the LSE use
    the undropped probabilities ``P``, ``y = (P * M / keep) @ v``, ``dS = P * (M * dP / keep - D)`` and dV
    takes the masked, scaled ``P``.  ``y_for_D`` replaces ``y`` in ``D = rowsum(dO * y)`` (the kernels form
    ``D`` from their own bf16 output).  ``allowed`` (bool ``[T, T]``) replaces the causal mask and ``v_src =
    (rows_from, index[T])`` makes queries ``>= rows_from`` read ``v[index]``: both exist for ``mutate``.

    Returns a namespace: ``y, lse2, D, dq, dk, dv``, the probabilities ``P``, and the denominators of the
    metric ``den_y, den_dq, den_dk, den_dv, den_D`` (``den_D = rowsum|dO * y|``)."""
    q, k, v, dO, y_for_D = _up(q, k, v, dO, y_for_D)
    T = q.shape[-2]
    allowed = causal_allowed(T) if allowed is None else allowed
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(~allowed, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    lse2 = ((m + torch.log(l)) / LN2).squeeze(-1)
    drop = None if mask is None else mask.to(F64) * float(inv_keep)
    Pd = P if drop is None else P * drop

    def rows_read(vv):          # [B, H, T, T] weights @ the V each query row reads
        if v_src is None:
            return lambda W: W @ vv
        r0, idx = v_src
        alt = vv[..., idx, :]
        return lambda W: torch.cat([W[..., :r0, :] @ vv, W[..., r0:, :] @ alt], -2)

    y = rows_read(v)(Pd)
    den_y = rows_read(v.abs())(Pd)
    yD = y if y_for_D is None else y_for_D
    D = (dO * yD).sum(-1)
    den_D = (dO * yD).abs().sum(-1)
    if v_src is None:
        dP = dO @ v.transpose(-1, -2)
    else:
        r0, idx = v_src
        dP = torch.cat([dO[..., :r0, :] @ v.transpose(-1, -2),
                        dO[..., r0:, :] @ v[..., idx, :].transpose(-1, -2)], -2)
    dPm = dP if drop is None else dP * drop
    dS = P * (dPm - D.unsqueeze(-1))
    A = P * (dPm.abs() + den_D.unsqueeze(-1))
    return SimpleNamespace(
        y=y, lse2=lse2, D=D, P=P,
        dq=SCALE * (dS @ k), dk=SCALE * (dS.transpose(-1, -2) @ q), dv=Pd.transpose(-1, -2) @ dO,
        den_y=den_y, den_D=den_D,
        den_dq=SCALE * (A @ k.abs()), den_dk=SCALE * (A.transpose(-1, -2) @ q.abs()),
        den_dv=Pd.transpose(-1, -2) @ dO.abs())


def decode_reference(q, K, V):
    """One query per (b, h) over ``n`` keys: ``q [B, H, 64]``, ``K, V [B, H, n, 64]`` -> ``(y, den_y)``,
    both ``[B, H, 64]`` fp64, with ``den_y = P @ |V|``."""
    q, K, V = _up(q, K, V)
    s = (K @ q.unsqueeze(-1)).squeeze(-1) * SCALE
    P = torch.softmax(s, -1).unsqueeze(-2)
    return (P @ V).squeeze(-2), (P @ V.abs()).squeeze(-2)


# ------------------------------------------------------------------------------------------ metric
# Absolute term of the metric's denominator.  bf16 and fp32 share an exponent range that ends near 1e-38 (and
# the kernels' bare v_exp_f32 flushes below 2^-126), so a probability of e^-100 is 0 in a kernel and 1e-44 in
# fp64: a row made of such terms only (`big` has them) cannot be held to a relative bound.  2^-100 is 1e8
# times the largest such loss at these shapes and 1e-25 of any row that carries weight.
UNDERFLOW = 2.0 ** -100


def row_errors(got, ref, den):
    """``||got_r - ref_r||_2 / (||den_r||_2 + UNDERFLOW)`` for every row (last dim = the row's 64 values).  A
    row whose ``den`` is exactly 0 must be exactly 0 in ``got``: its error is 0 if so and ``inf`` otherwise.
    A non-finite ``got`` row has error ``inf``."""
    got, ref, den = _up(got, ref, den)
    num = (got - ref).norm(dim=-1)
    dn = den.norm(dim=-1)
    err = num / (dn + UNDERFLOW)
    zero = dn == 0
    err = torch.where(zero, torch.where(got.abs().amax(-1) == 0, 0.0, float("inf")).to(F64), err)
    return torch.where(torch.isfinite(got).all(-1), err, torch.full_like(err, float("inf")))


def row_error(got, ref, den):
    """The score of a check: the maximum of ``row_errors`` over all ``(b, h, row)``."""
    return row_errors(got, ref, den).max().item()


def worst_row(got, ref, den):
    """``(error, (b, h, row))`` of the worst row, for failure messages."""
    e = row_errors(got, ref, den)
    i = int(e.flatten().argmax())
    return e.flatten()[i].item(), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), e.shape))


def scores(got, ref):
    """Metric of ``y, dq, dk, dv`` of ``got`` (anything with those attributes) against a ``reference``."""
    return {n: row_error(getattr(got, n), getattr(ref, n), getattr(ref, "den_" + n)) for n in ("y", "dq", "dk", "dv")}


def old_metric(a, b):
    """``max|a - b| / max|b|`` over the whole tensor: what the older attention tests use."""
    a, b = _up(a, b)
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


# ------------------------------------------------------------------------------------------ input families
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _units(g, *shape):
    u = _randn(g, *shape)
    return u / u.norm(dim=-1, keepdim=True)


PEAK = math.sqrt(40.0 / SCALE)     # |q| = |k| = a with a^2 * scale = 40


def _bf(*ts):
    return tuple(t.to(BF16) for t in ts)


def gauss(s):
    def f(B, H, T, seed):
        g = _gen(seed)
        return _bf(s * _randn(g, B, H, T, HD), _randn(g, B, H, T, HD), _randn(g, B, H, T, HD))
    return f


def _peak_at(offset):
    """Score about 40 where key == query - offset (rows without such a key keep random scores), about
    N(0, 5) elsewhere: q[t] = a u[t - offset], k[t] = a u[t] with random unit vectors u.  The rows of v are
    random directions of one length (8, the typical length of a randn row), so that no key's value is small
    against the others: a row that gains or loses its peak moves by its whole magnitude."""
    def f(B, H, T, seed):
        g = _gen(seed)
        u = _units(g, B, H, T, HD)
        other = _units(g, B, H, T, HD)
        t = torch.arange(T)
        src = t - offset
        ok = (src >= 0) & (src < T)
        qd = torch.where(ok[:, None], u[..., src.clamp(0, T - 1), :], other)
        return _bf(PEAK * qd, PEAK * u, math.sqrt(HD) * _units(g, B, H, T, HD))
    return f


leak = _peak_at(-1)                 # the peak sits on the first masked key, q + 1


def needle(d):
    return _peak_at(d)


def first(B, H, T, seed):
    """Peak at key 0 for every query: tile 0 sets the running max and nothing later rescales."""
    g = _gen(seed)
    u = _units(g, B, H, T, HD)
    q = PEAK * u[..., :1, :] + _randn(g, B, H, T, HD)
    return _bf(q, PEAK * u, _randn(g, B, H, T, HD))


def _ramp(ksign, alternate):
    def f(B, H, T, seed):
        g = _gen(seed)
        q, k, v = _randn(g, B, H, T, HD), _randn(g, B, H, T, HD), _randn(g, B, H, T, HD)
        t = torch.arange(T, dtype=F64)
        q[..., 63] = torch.where(torch.arange(T) % 2 == 1, -4.0, 4.0).to(F64) if alternate else 4.0
        k[..., 63] = ksign * (t / 16).to(BF16).to(F64)
        return _bf(q, k, v)
    return f


incr = _ramp(1.0, False)            # the running max grows on every tile
decr = _ramp(-1.0, False)           # ... never after the first
split = _ramp(1.0, True)            # even queries as incr, odd queries as decr: both kinds in every wave


def uniform(B, H, T, seed):
    """q == 0, integer v: y[t] = mean(v[0..t]) and lse2[t] = log2(t + 1)."""
    g = _gen(seed)
    v = torch.randint(-8, 9, (B, H, T, HD), generator=g).to(F64)
    return _bf(torch.zeros(B, H, T, HD, dtype=F64), _randn(g, B, H, T, HD), v)


def big(B, H, T, seed):
    """Scaled scores up to about +-200, and keys in identical pairs, so a row's maximum is an exact tie
    whenever both keys of the pair are visible."""
    g = _gen(seed)
    q, k, v = 8 * _randn(g, B, H, T, HD), 8 * _randn(g, B, H, T, HD), _randn(g, B, H, T, HD)
    k[..., 1::2, :] = k[..., 0::2, :]
    return _bf(q, k, v)


FAMILIES = {"gauss0.25": gauss(0.25), "gauss1": gauss(1.0), "gauss4": gauss(4.0), "leak": leak,
            **{f"needle{d}": needle(d) for d in (0, 1, 63, 64, 127, 128)},
            "first": first, "incr": incr, "decr": decr, "split": split, "uniform": uniform, "big": big}


def make(family, B, H, T, seed=0):
    """bf16 ``q, k, v, dO`` of a family (``dO`` is ``randn``), each ``[B, H, T, 64]``."""
    q, k, v = FAMILIES[family](B, H, T, seed)
    dO = torch.randn(B, H, T, HD, generator=_gen(seed + 7919), dtype=F64).to(BF16)
    return q, k, v, dO


# ------------------------------------------------------------------------------------------ emulation
def _r(x):
    return x.to(BF16).to(F64)


def emulate(q, k, v, dO, mask=None, inv_keep=1.0):
    """The kernels' rounding points in fp64 arithmetic: the unnormalised P is rounded to bf16 before PV while
    ``l`` is summed unrounded, O is rounded to bf16 and ``D`` comes from that rounded O; the backward takes
    ``P = exp2(s - lse2)``, rounds P (masked and scaled) and dS to bf16 before their matmuls and rounds the
    outputs to bf16.  For the noise floor of the metric only -- never an expected value."""
    q, k, v, dO = _up(q, k, v, dO)
    T = q.shape[-2]
    allowed = causal_allowed(T)
    s = ((q @ k.transpose(-1, -2)) * SCALE).masked_fill(~allowed, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    keep = None if mask is None else mask.to(F64)
    y = _r((_r(e if keep is None else e * keep) @ v) * (float(inv_keep) / l))
    lse = m + torch.log(l)
    D = (dO * y).sum(-1, keepdim=True)
    P = torch.exp(s - lse)
    dP = dO @ v.transpose(-1, -2)
    if keep is not None:
        dP = dP * keep * float(inv_keep)
    dS = _r(P * (dP - D))
    Pd = _r(P if keep is None else P * keep * float(inv_keep))
    return SimpleNamespace(y=y, lse2=(lse / LN2).squeeze(-1), D=D.squeeze(-1),
                           dq=_r(SCALE * (dS @ k)), dk=_r(SCALE * (dS.transpose(-1, -2) @ q)),
                           dv=_r(Pd.transpose(-1, -2) @ dO))


# ------------------------------------------------------------------------------------------ mutations
MUTATIONS = ("self_excluded", "next_included", "one_in_64_dropped", "stale_v_tile")


def mutate(mask, kind, rows_from):
    """A deliberately wrong version of the causal mask ``mask`` (bool ``[T, T]``) for query rows ``>=
    rows_from``, as keyword arguments for ``reference``: ``self_excluded`` hides the query's own key (row 0
    keeps it), ``next_included`` admits key ``q + 1``, ``one_in_64_dropped`` hides keys with ``k % 64 == 37``
    and ``stale_v_tile`` makes keys 192..255 read the V rows of keys 128..191."""
    T = mask.shape[0]
    out = mask.clone()
    rows = torch.arange(T) >= rows_from
    t = torch.arange(T)
    if kind == "self_excluded":
        sel = rows & (t > 0)
        out[t[sel], t[sel]] = False
    elif kind == "next_included":
        sel = rows & (t < T - 1)
        out[t[sel], t[sel] + 1] = True
    elif kind == "one_in_64_dropped":
        out[rows.nonzero()[:, 0][:, None], t[t % 64 == 37][None, :]] = False
    elif kind == "stale_v_tile":
        idx = t.clone()
        idx[192:256] = t[128:192]
        return dict(allowed=out, v_src=(int(rows_from), idx))
    else:
        raise ValueError(f"mutate: unknown kind {kind!r}")
    return dict(allowed=out)


# ------------------------------------------------------------------------------------------ tables
def _tables(T=1024, rows_from=896):
    """The figures of profiles/attention_tests/README.md: ``python tests/attention_ref.py``."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pytorch_distributed_example_amd.ops import DeviceRNG
    from pytorch_distributed_example_amd.ops import rng as R

    outs = ("y", "dq", "dk", "dv")
    worst = 0.0
    print(f"emulation floor, T = {T}, B = H = 1\n| family | p | y | dq | dk | dv |\n|---|---|---|---|---|---|")
    for p in (0.0, 0.1):
        for name in FAMILIES:
            q, k, v, dO = make(name, 1, 1, T)
            kw = {}
            if p:
                kw = dict(mask=R.attention_mask(DeviceRNG(5).next(), 3, 1, 1, T, p), inv_keep=R.inv_keep(p, "attention"))
            em = emulate(q, k, v, dO, **kw)
            sc = scores(em, reference(q, k, v, dO, y_for_D=em.y, **kw))
            worst = max(worst, *sc.values())
            print(f"| {name} | {p} | " + " | ".join(f"{sc[n]:.5f}" for n in outs) + " |")
    print(f"worst {worst:.5f}; FLOOR {FLOOR}, BOUND {BOUND:.5f}\n")
    print(f"mutations of rows >= {rows_from}, T = {T}: new metric | max|a-b| / max|b|")
    print("| family | mutation | y | dq | dk | dv | old y | old dq | old dk | old dv |\n|" + "---|" * 10)
    for name in FAMILIES:
        q, k, v, dO = make(name, 1, 1, T)
        ref = reference(q, k, v, dO)
        for kind in MUTATIONS:
            mu = reference(q, k, v, dO, **mutate(causal_allowed(T), kind, rows_from))
            sc = scores(mu, ref)
            old = [old_metric(getattr(mu, n), getattr(ref, n)) for n in outs]
            print(f"| {name} | {kind} | " + " | ".join(f"{min(sc[n], 999):.4f}" for n in outs) + " | " +
                  " | ".join(f"{min(o, 999):.4f}" for o in old) + " |")


if __name__ == "__main__":
    _tables()
