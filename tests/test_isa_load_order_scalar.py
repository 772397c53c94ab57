"""tools/isa_load_order.py --scalar: the parsing half (no compiler, no GPU) on a hand-written listing."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_load_order", os.path.join(ROOT, "tools", "isa_load_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# a prologue in the shape of an optimizer kernel: arguments, a dependent memory word, more arguments,
# then the element loop with one argument re-fetched inside it
BODY = """
\ts_load_dwordx4 s[4:7], s[0:1], 0x0
\ts_load_dwordx2 s[8:9], s[0:1], 0x40
\ts_load_dword s10, s[0:1], 0x60
\ts_waitcnt lgkmcnt(0)
\ts_load_dwordx2 s[12:13], s[8:9], 0x0
\ts_waitcnt lgkmcnt(0)
\ts_cmp_lg_u64 s[12:13], 0
\ts_cbranch_scc1 .LBB0_2
\ts_load_dword s14, s[0:1], 0x70
\ts_waitcnt lgkmcnt(0)
.LBB0_2:
\ts_load_dwordx2 s[16:17], s[0:1], 0x8
\tds_read_b32 v9, v5
\ts_waitcnt lgkmcnt(1)
\tglobal_load_dwordx4 v[0:3], v[6:7], off
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tglobal_store_dwordx4 v[6:7], v[0:3], off
\ts_cbranch_vccnz .LBB0_2
\ts_endpgm
""".splitlines()


def test_scalar_loads_beside_the_lgkm_waits():
    t = _tool()
    assert t.order(BODY, scalar=True) == [("entry", "3s g0 1s g0 br 1s g0"), (".LBB0_2", "1s g1 1L w0 g0 1S br")]


def test_scalar_and_lds_together():
    t = _tool()
    assert t.order(BODY, lds=True, scalar=True) == [("entry", "3s g0 1s g0 br 1s g0"),
                                                    (".LBB0_2", "1s 1r g1 1L w0 g0 1S br")]


def test_listings_without_the_option_are_unchanged():
    t = _tool()
    assert t.order(BODY) == [(".LBB0_2", "1L w0 1S br")]
    assert t.order(BODY, lds=True) == [("entry", "2g0 br g0"), (".LBB0_2", "1r g1 1L w0 g0 1S br")]
