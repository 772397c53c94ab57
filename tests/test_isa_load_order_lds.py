"""tools/isa_load_order.py --lds: the parsing half (no compiler, no GPU) on a hand-written listing."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_load_order", os.path.join(ROOT, "tools", "isa_load_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BODY = """
\tglobal_load_dword v1, v[2:3], off
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tds_write_b128 v4, v[8:11]
\ts_waitcnt lgkmcnt(0)
\ts_barrier
\tds_read_b128 v[8:11], v4
\tds_read2_b32 v[12:13], v5 offset1:1
\tds_read_b32 v14, v5 offset:2312
\ts_waitcnt lgkmcnt(2)
\tv_mfma_f32_16x16x4_f32 v[0:3], v8, v12, v[0:3]
\ts_waitcnt lgkmcnt(1)
\tv_mfma_f32_16x16x4_f32 v[0:3], v9, v13, v[0:3]
\tv_mov_b32_dpp v16, v6 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1
\tds_swizzle_b32 v13, v6 offset:swizzle(SWAP,4)
\tds_bpermute_b32 v7, v20, v6
\tds_add_f32 v4, v7
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v[2:3], v7, off
\ts_endpgm
""".splitlines()


def test_lds_tokens_beside_the_plain_ones():
    t = _tool()
    assert t.order(BODY, lds=True) == [("entry", "1L w0 g0 1d g0 BAR 3r g2 1M g1 1M 3x g0 1S")]


def test_listing_without_the_option_is_unchanged():
    t = _tool()
    assert t.order(BODY) == [("entry", "1L w0 BAR 2M 1S")]
