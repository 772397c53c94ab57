"""Beam search on the GPU: the table-indirect decode attention against the plain kernel on a gathered cache (bit for
bit), the selection kernels against ``beam_step_reference``, and ``GPT.generate(num_beams=)`` against a teacher-forced
CPU fp32 twin, against a host replay of every step, and against its own equivalences."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.models.gpt2 import DecodeSession
from pytorch_distributed_example_amd.ops import decode as D

import beam_cases as BC
import generate_cases as GC
from test_generate_gpu import _Cfg, _random_cache

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
GAP = BC.GAP
# The device score is an fp32 row maximum, a sum of at most 50257 exponentials and one logf (bounded at 4e-6 and 1e-5
# by the sampler test) plus two fp32 additions on magnitudes below 64 (ulp 3.8e-6): 3e-5 is where to start asking why.
SCORE_ALERT = 3e-5


# --------------------------------------------------------------------------------------- attention through the table
def test_attention_through_table_is_the_plain_kernel_on_a_gathered_cache():
    B, K, H, Tmax = 2, 3, 2, 512
    R = B * K
    cache = _random_cache(R, Tmax, seed=11)
    before = cache.data.clone()
    g = torch.Generator().manual_seed(12)
    grp = (torch.arange(R) // K * K)[:, None]
    for n, p in enumerate((0, 1, 127, 128, 129, 255, 256, 511)):
        step = n % 2 + 2 * (n // 4)                                  # both halves of the table
        table = D.beam_table(B, K, Tmax)
        table[step & 1, :R, :p] = (grp + torch.randint(0, K, (R, p), generator=g)).to(torch.uint8)
        table[(step & 1) ^ 1, :R] = (grp + torch.randint(0, K, (R, Tmax), generator=g)).to(torch.uint8)
        table = table.to(dev)
        gathered = D.KVCache(_Cfg, R, Tmax, dev)
        gathered.data.copy_(before)
        t = torch.arange(p, device=dev)
        for r in range(R):
            gathered.data[0, :, r, :, :p] = before[0, :, table[step & 1, r, :p].long(), :, t].permute(1, 2, 0, 3)
        qkv = torch.randn(R, 3 * H * 64, generator=g).to(dev, BF16)
        state = D.DecodeState(dev, pos=p, step=step)
        words = state.buf.clone()
        y = D.decode_attention(qkv, cache, 0, state, beam_table=table)
        assert torch.equal(y, D.decode_attention(qkv, gathered, 0, state)), p
        # the cache differs from before in row r, position p only, which holds the new K and V bit for bit
        expect = before.clone()
        expect[0, 0, :, :, p] = qkv[:, H * 64:2 * H * 64].reshape(R, H, 64)
        expect[0, 1, :, :, p] = qkv[:, 2 * H * 64:].reshape(R, H, 64)
        assert torch.equal(cache.data, expect), p
        assert torch.equal(state.buf, words)
        cache.data.copy_(before)
        assert torch.equal(D.decode_attention(qkv, cache, 0, state, beam_table=table), y), p      # a second run
        cache.data.copy_(before)


# --------------------------------------------------------------------------------------- the selection kernels
def _buffers(B, K, V, Vp, S, fin, ln, step, T0=6, n_new=4, eos=BC.EOS):
    """Beam buffers in the middle of a generation: at ``step``, with the rows' ``S``, flags and lengths given."""
    bb = D.BeamBuffers(D.BeamConfig(K, 1.0, eos), torch.zeros(B, T0, dtype=torch.int64, device=dev), None, n_new, V, Vp,
                       dev, T0 + n_new)
    bb.state.reset(pos=T0 - 1 + step, step=step)
    R = B * K
    bb.score.copy_(torch.as_tensor(S, dtype=torch.float32))
    bb.state.finished[:R] = torch.as_tensor(fin).to(dev, torch.int32)
    bb.len.copy_(torch.as_tensor(ln, dtype=torch.int32))
    return bb


def _run_step(B, K, V, Vp, logits, S, fin, ln, ref, step=1):
    """One device step against ``ref`` = ``beam_step_reference``'s result: exact choice and order, scores within
    ``GAP``, and everything else the step writes by the rule.  Returns the largest score difference."""
    R = B * K
    fin = torch.as_tensor(fin).bool()
    ln = torch.as_tensor(ln, dtype=torch.int64)
    bb = _buffers(B, K, V, Vp, S, fin, ln, step)
    # a table as it is in the middle of a generation: any row of the group per position, the halves different
    g = torch.Generator().manual_seed(R + step)
    grp = (torch.arange(R) // K * K)[:, None, None]
    bb.table[:, :R] = (grp + torch.randint(0, K, (R, 2, bb.table.shape[2]), generator=g)).transpose(0, 1).to(dev, torch.uint8)
    words, table = bb.state.buf.clone(), bb.table.clone()
    nxt = D.beam_step(logits.to(dev), bb)
    parent, tok, score, info = ref
    dp, dt, ds = (x[step].cpu().reshape(B, K) for x in (bb.parent, bb.tok, bb.score_trace))
    err = float((ds.double() - score).abs().max())
    assert torch.equal(dp.long(), parent) and torch.equal(dt.long(), tok), (dp, parent, dt, tok)
    assert err <= GAP, err
    src = (torch.arange(B)[:, None] * K + parent).reshape(R)
    assert torch.equal(nxt.cpu(), tok.reshape(R)) and torch.equal(bb.score.cpu(), ds.reshape(R))
    assert torch.equal(bb.len.cpu().long(), ln[src] + (~fin[src]).long())
    assert torch.equal(bb.state.finished[:R].cpu().bool(), fin[src] | (tok.reshape(R) == BC.EOS))
    for s in range(bb.n_new):
        if s != step:
            assert not bb.tok[s].any() and not bb.parent[s].any() and not bb.score_trace[s].any()
    # position and step advanced, the draw number and the offsets as they were
    want = words.clone()
    want[D._POS] += 1
    want[D._STEP] += 1
    want[D._FIN:D._FIN + R] = bb.state.finished[:R]
    assert torch.equal(bb.state.buf, want)
    # the table: the half of this step's parity is untouched, the other one follows the rule up to position p
    p = int(words[D._POS])
    rd, wr = step & 1, (step & 1) ^ 1
    assert torch.equal(bb.table[rd], table[rd])
    got = bb.table[wr].cpu()
    for r in range(R):
        assert torch.equal(got[r, :p], table[rd, int(src[r]), :p].cpu()) and int(got[r, p]) == int(src[r]), r
    assert torch.equal(bb.table[wr, R:], table[wr, R:])
    return err, bb


@pytest.mark.parametrize("B,K,V,Vp", BC.KERNEL_SHAPES)
def test_beam_step_matches_reference(B, K, V, Vp):
    worst = 0.0
    for i in range(BC.N_KERNEL_INPUTS):
        logits, S, fin = BC.kernel_input(i, B, K, V, Vp)
        ref = BC.kernel_reference(i, B, K, V, Vp)
        assert float(ref[3]["gap"].min()) >= GAP                     # asserted >= MIN_GAP on the CPU: exact, none left out
        err, _ = _run_step(B, K, V, Vp, logits, S, fin, 2 + torch.arange(B * K) % 3, ref, step=1 + i % 2)
        worst = max(worst, err)
    print(f"(B, K, V) = {(B, K, V)}: largest |device - fp64| score difference {worst:.3e}")
    assert worst <= SCORE_ALERT, worst


@pytest.mark.parametrize("name", sorted(BC.hand_cases()))
def test_hand_made_steps(name):
    c = BC.hand_cases()[name]
    ref = BC.hand_reference(c)
    err, bb = _run_step(c["B"], c["K"], c["V"], c["Vp"], c["logits"], c["S"], c["fin"], c["len"], ref,
                        step=0 if c["first"] else 1)
    if name == "step0":                                              # every beam descends from the prompt's row
        assert bb.len.cpu().tolist() == [1] * 6 and not bb.parent[0].any()
    if name == "all_finished":                                       # the scores stand, bit for bit
        assert bb.score.cpu().tolist() == [-1.0, -2.0, -3.0, -4.0] and bb.len.cpu().tolist() == [5, 3, 2, 4]
    if name == "cross_beam_tie":                                     # identical rows give identical bits
        assert bb.score[0].item() == bb.score[1].item()
    if name == "chooses_eos":
        assert bb.len.cpu().tolist()[:2] == [5, 2] and bb.state.finished[:2].cpu().tolist() == [1, 1]


# --------------------------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def twins():
    """bf16 GPU model and its fp32 CPU twin (``beam_cases.twin``): identical, bf16-representable weights."""
    c = BC.twin()
    g = build_gpt2(GC.tiny_cfg(), seed=0, device=dev)
    with torch.no_grad():
        g.transformer.ln_f.weight.fill_(BC.LN_F_SCALE)
    assert all(torch.equal(pc, pg.float().cpu()) for pc, pg in zip(c.parameters(), g.parameters()))
    return g.eval(), c


_RUNS = {}


def _generation(g, case, after_prefill=None, **kw):
    """One GPU beam search of ``BC.HYP_CASES[case]`` with everything it returns, computed once per setting."""
    key = (case, after_prefill, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = _generate(g, case, after_prefill, **kw)
    return _RUNS[key]


def _generate(g, case, after_prefill, **kw):
    B, K, T0, n_new, seed = BC.HYP_CASES[case]
    idx = BC.prompt(B, T0, seed)
    tr = {}
    out, scores, lg = g.generate(idx.to(dev), n_new, num_beams=K, return_beams=True, return_logits=True,
                                 _beam_trace=tr, _after_prefill=after_prefill, **kw)
    torch.cuda.synchronize()
    return idx, out.cpu(), scores.cpu(), lg.float().cpu(), {k: v.cpu() for k, v in tr.items()}


def _ancestors(tr, b, K, j):
    """The rows ``[n_new]`` that held hypothesis ``j`` (its last row) of group ``b`` after every step."""
    n = tr["tok"].shape[0]
    rows, row = [0] * n, j
    for s in range(n - 1, -1, -1):
        rows[s] = row
        row = int(tr["parent"][s, b * K + row])
    return rows


def _twin_failures(g, c, case, after_prefill=None):
    B, K, T0, n_new, _ = BC.HYP_CASES[case]
    idx, out, scores, lg, tr = _generation(g, case, after_prefill)
    assert out.shape == (B, K, T0 + n_new) and scores.shape == (B, K) and lg.shape == (B * K, n_new, 1000)
    order, _ = D.beam_rank_reference(tr["S"], tr["len"], K, 1.0)
    fails = []
    for b in range(B):
        for i in range(K):
            assert torch.equal(out[b, i, :T0], idx[b])
            rows = _ancestors(tr, b, K, int(order[b, i]))
            assert out[b, i, T0:].tolist() == [int(tr["tok"][s, b * K + rows[s]]) for s in range(n_new)]
            with torch.no_grad():
                ref = c(out[b, i:i + 1, :-1])[0]                     # teacher forcing: the twin sees the hypothesis
            for s in range(n_new):
                src = b * K + int(tr["parent"][s, b * K + rows[s]])  # the row whose logits the token was chosen from
                x, y = lg[src, s].double(), ref[T0 - 1 + s].double()
                cs = F.cosine_similarity(x, y, dim=0).item()
                e = ((x - y).norm() / y.norm()).item()
                if not (cs >= 0.995 and e < 3e-2):
                    fails.append(f"prompt {b} rank {i} step {s}: cos {cs:.5f}, rel L2 err {e:.3e}")
    return fails


@pytest.mark.parametrize("case", range(len(BC.HYP_CASES)))
def test_hypotheses_match_teacher_forced_twin(twins, case):
    fails = _twin_failures(*twins, case)
    assert not fails, fails


def _zero_position_2(cache):
    cache.data[:, :, :, :, 2] = 0


def test_twin_check_catches_a_zeroed_cache_position(twins):
    assert _twin_failures(*twins, 0, _zero_position_2), "a zeroed KV cache position went unnoticed"


def _replay(tr, lg, B, K, V, eos):
    """Every step again on the host with ``beam_step_reference``, fed the device's own previous scores.  Returns the
    number of steps whose gap is below ``GAP`` and the largest score difference."""
    n_new, R = tr["tok"].shape
    S, fin = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.bool)
    close, worst = 0, 0.0
    for s in range(n_new):
        parent, tok, score, info = D.beam_step_reference(lg[:, s], V, K, S, fin, eos, first=s == 0, return_info=True)
        dp, dt, ds = (tr[k][s].reshape(B, K) for k in ("parent", "tok", "score"))
        x = lg[:, s].double()
        logp = x - torch.logsumexp(x, 1, keepdim=True)
        for b in range(B):
            rows = b * K + dp[b].long()
            exact = torch.where(fin[rows], S[rows], S[rows] + logp[rows, dt[b].long()])     # fp64 scores of the chosen
            worst = max(worst, float((ds[b].double() - exact).abs().max()))
            assert float((ds[b].double() - exact).abs().max()) <= GAP, (s, b)
            if info["gap"][b] >= GAP:
                assert torch.equal(dp[b].long(), parent[b]) and torch.equal(dt[b].long(), tok[b]), (s, b)
                continue
            close += 1                   # a closer step must still be valid
            assert (exact[1:] - exact[:-1] <= GAP).all(), (s, b)
            cand = torch.full((K, V), -np.inf, dtype=torch.float64)
            for k in range(1 if s == 0 else K):
                r = b * K + k
                if fin[r]:
                    cand[k, eos] = S[r]
                else:
                    cand[k] = S[r] + logp[r]
            cand[dp[b].long(), dt[b].long()] = -np.inf
            assert float(cand.max()) - float(exact.min()) <= GAP, (s, b)
        src = (torch.arange(B)[:, None] * K + dp.long()).reshape(R)
        fin = fin[src] | ((dt.reshape(R) == eos) if eos is not None else False)
        S = ds.reshape(R).double()                                   # the device's own scores: nothing accumulates
    return close, worst


@pytest.mark.parametrize("case", range(len(BC.HYP_CASES)))
def test_selection_replayed_on_the_host(twins, case):
    B, K, T0, n_new, _ = BC.HYP_CASES[case]
    idx, out, scores, lg, tr = _generation(twins[0], case)
    close, worst = _replay(tr, lg, B, K, 1000, None)
    print(f"case {BC.HYP_CASES[case]}: {close} close step(s), largest |device - fp64| score difference {worst:.3e}")
    assert close <= 1                                                # a cap, not a measurement
    assert worst <= SCORE_ALERT, worst
    # the ranked scores and tokens from the trace
    order, ranked = D.beam_rank_reference(tr["S"], tr["len"], K, 1.0)
    assert np.allclose(scores.double().numpy(), ranked.numpy(), rtol=1e-6, atol=0)
    assert (tr["len"] == n_new).all() and not tr["finished"].any()


def test_graph_replay_equals_eager(twins):
    a, b = _generation(twins[0], 0), _generation(twins[0], 0, use_graph=False)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert all(torch.equal(a[4][k], b[4][k]) for k in a[4])


def test_unreferenced_cache_slots_are_never_read(twins):
    B, K, T0, _, _ = BC.HYP_CASES[0]

    def poison(cache):
        keep = torch.zeros(cache.data.shape[2], cache.data.shape[4], dtype=torch.bool, device=dev)
        keep[::K, :T0] = True                                        # what the initial table references
        cache.data.masked_fill_(~keep[None, None, :, None, :, None], float("nan"))
        assert cache.data.isnan().any() and not cache.data[:, :, ::K, :, :T0].isnan().any()

    a, b = _generation(twins[0], 0), _generation(twins[0], 0, poison)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_ragged_prompts_equal_batches_of_one_length(twins):
    g, _ = twins
    lens, K, n_new = BC.RAGGED_LENS, BC.RAGGED_K, BC.RAGGED_NEW
    B = len(lens)
    idx = BC.prompt(B, max(lens), BC.RAGGED_SEED).to(dev)
    kw = dict(num_beams=K, return_beams=True, return_logits=True, pad_token_id=3)
    out, sc, lg = g.generate(idx, n_new, prompt_lens=lens, **kw)
    assert out.shape == (B, K, max(lens) + n_new)
    for b, n in enumerate(lens):
        same = idx[b:b + 1, :n].repeat(B, 1)                         # the same B, one prompt length
        o1, s1, l1 = g.generate(same, n_new, **kw)
        assert torch.equal(out[b, :, :n + n_new], o1[b]) and (out[b, :, n + n_new:] == 3).all(), b
        assert torch.equal(sc[b], s1[b]) and torch.equal(lg[b * K:(b + 1) * K], l1[b * K:(b + 1) * K]), b


def test_eos_freezing_and_final_ranking(twins):
    g, _ = twins
    B, K, T0, n_new = 2, 4, 5, 8
    V = 1000
    idx = BC.prompt(B, T0, 1).to(dev)
    free = g.generate(idx, n_new, num_beams=K, return_beams=True)[0]
    eos = int(free[0, 1, T0 + 1])                                    # the second token of a surviving hypothesis
    for lp in (0.0, 1.0, 2.0):
        tr = {}
        out, sc, lg = g.generate(idx, n_new, num_beams=K, length_penalty=lp, eos_token_id=eos, return_beams=True,
                                 return_logits=True, _beam_trace=tr)
        tr = {k: v.cpu() for k, v in tr.items()}
        out, sc = out.cpu(), sc.cpu()
        close, _ = _replay(tr, lg.float().cpu(), B, K, V, eos)
        assert close <= 1
        fin, ln = tr["finished"].bool(), tr["len"].long()
        assert fin.any() and (ln[fin] < n_new).any(), "no beam finished early"
        # recomputed on the host from the trace: lengths, flags, order, scores and tokens
        f, n = torch.zeros(B * K, dtype=torch.bool), torch.zeros(B * K, dtype=torch.int64)
        for s in range(n_new):
            src = (torch.arange(B)[:, None] * K + tr["parent"][s].reshape(B, K).long()).reshape(B * K)
            frozen = f[src]
            assert (tr["tok"][s][frozen] == eos).all()
            if s:
                assert torch.equal(tr["score"][s][frozen], tr["score"][s - 1][src][frozen])     # the score stands
            n = n[src] + (~frozen).long()
            f = frozen | (tr["tok"][s] == eos)
        assert torch.equal(f, fin) and torch.equal(n, ln)
        order, ranked = D.beam_rank_reference(tr["S"], ln, K, lp)
        assert np.allclose(sc.double().numpy(), ranked.numpy(), rtol=1e-6, atol=0)
        for b in range(B):
            for i in range(K):
                rows = _ancestors(tr, b, K, int(order[b, i]))
                assert out[b, i, T0:].tolist() == [int(tr["tok"][s, b * K + rows[s]]) for s in range(n_new)]
        assert torch.equal(g.generate(idx, n_new, num_beams=K, length_penalty=lp, eos_token_id=eos).cpu(), out[:, 0])


def test_one_beam_is_the_default_call(twins):
    g, _ = twins
    idx = BC.prompt(3, 6, 2).to(dev)
    for kw in (dict(temperature=0.8, top_k=40, seed=11), dict(temperature=0.0)):
        a, la = g.generate(idx, 6, return_logits=True, **kw)
        b, lb = g.generate(idx, 6, return_logits=True, num_beams=1, length_penalty=2.0, **kw)
        assert torch.equal(a, b) and torch.equal(la, lb)
    with torch.no_grad():
        ses = DecodeSession(g, idx, 3, beam=D.BeamConfig(1))
    assert ses.beam is None and ses._table is None and isinstance(ses.buffers, D.SampleBuffers)


def test_more_than_sixteen_rows(twins):
    g, _ = twins
    with pytest.raises(NotImplementedError):
        g.generate(BC.prompt(3, 4, 0).to(dev), 2, num_beams=6)
    out = g.generate(BC.prompt(4, 4, 0).to(dev), 2, num_beams=4)     # 16 rows fit
    assert out.shape == (4, 6)
