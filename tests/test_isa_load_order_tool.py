"""tools/isa_load_order.py: the parsing half (no compiler, no GPU) on a hand-written listing."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_load_order", os.path.join(ROOT, "tools", "isa_load_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ASM = """
\t.globl\t_Z3fooPf
_Z3fooPf:                               ; @_Z3fooPf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\tglobal_load_dwordx4 v[4:7], v[0:1], off
\tglobal_load_dwordx4 v[8:11], v[0:1], off offset:64
\tbuffer_load_dword v12, v2, s[8:11], 0 offen
\ts_waitcnt vmcnt(2)
\tv_mfma_f32_16x16x4_f32 a[0:3], v4, v8, a[0:3]
\tv_mfma_f32_16x16x4_f32 a[0:3], v5, v9, a[0:3]
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tds_write_b32 v3, v12
\ts_barrier
\ts_cbranch_execz .LBB0_2
; %bb.1:
\tglobal_store_dword v[0:1], v4, off
\tglobal_atomic_add_f32 v[0:1], v5, off
.LBB0_2:
\ts_cbranch_scc1 .LBB0_3
.LBB0_3:
\ts_endpgm
\t.section\t.rodata
\t.amdhsa_kernel _Z3fooPf
\t.end_amdhsa_kernel
\t.text
.Lfunc_end0:
"""

REMARKS = """
k.hip:3:1: remark: Function Name: _Z3fooPf [-Rpass-analysis=kernel-resource-usage]
k.hip:3:1: remark:     TotalSGPRs: 18 [-Rpass-analysis=kernel-resource-usage]
k.hip:3:1: remark:     VGPRs: 13 [-Rpass-analysis=kernel-resource-usage]
k.hip:3:1: remark:     AGPRs: 4 [-Rpass-analysis=kernel-resource-usage]
k.hip:3:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
k.hip:3:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
k.hip:3:1: remark:     LDS Size [bytes/block]: 256 [-Rpass-analysis=kernel-resource-usage]
"""


def test_order_of_a_listing():
    t = _tool()
    bodies = t.kernel_bodies(ASM)
    assert list(bodies) == ["_Z3fooPf"]
    # lgkmcnt-only waits and LDS writes are not global-memory events; branch-only blocks are dropped
    assert t.order(bodies["_Z3fooPf"]) == [("entry", "3L w2 2M w0 BAR br 1S 1A")]
    assert t.order(bodies["_Z3fooPf"], all_blocks=True) == [("entry", "3L w2 2M w0 BAR br 1S 1A"), (".LBB0_2", "br")]


def test_resource_remarks():
    t = _tool()
    res = t.resources(REMARKS)
    assert res == {"_Z3fooPf": {"TotalSGPRs": "18", "VGPRs": "13", "AGPRs": "4", "ScratchSize [bytes/lane]": "0",
                                "Occupancy [waves/SIMD]": "8", "LDS Size [bytes/block]": "256"}}


def test_run_length_encoding():
    t = _tool()
    assert t.rle(["L"] * 27 + ["w23"] + ["M"] * 4 + ["w0", "w0", "BAR", "S"]) == "27L w23 4M 2w0 BAR 1S"
