#!/usr/bin/env python
"""Order of memory operations, waits and MFMAs in compiled kernels (CPU only, no GPU needed).

Compiles one ``.hip`` file to gfx950 assembly with the project's flags
(``hipcc -O3 --offload-arch=gfx950 -S --cuda-device-only -Rpass-analysis=kernel-resource-usage``)
and, for every kernel whose name contains one of the given substrings, prints

* the register / scratch / occupancy figures of the resource-usage remarks, and
* the run-length-encoded sequence of global loads (``L``), stores (``S``), atomics (``A``),
  ``s_waitcnt vmcnt(n)`` (``w<n>``), MFMAs (``M``), barriers (``BAR``) and conditional branches
  (``br``), one line per basic block that holds any of them (blocks with nothing but branches
  are left out unless ``--all-blocks`` is given).  With ``--lds`` the LDS side is listed too:
  ``ds_read*`` (``r``), ``ds_write*`` (``d``), lane exchanges -- ``ds_bpermute`` / ``ds_permute`` /
  ``ds_swizzle`` and DPP moves -- (``x``) and ``s_waitcnt lgkmcnt(n)`` (``g<n>``; a wait on both
  counters prints ``w<n> g<m>``).  With ``--scalar`` the scalar loads (``s_load_*``) are listed as ``s``
  next to the same ``g<n>`` waits, so a prologue that fetches its kernel arguments in several
  dependent rounds shows ``7s g0 1s g0 br 4s g0 ...`` ahead of its first ``L``.

A kernel that issues all its loads before the first MFMA shows ``26L`` ahead of the first ``M``;
one that the compiler serialised shows ``4L w0 8M 4L w0 ...``.

    python tools/isa_load_order.py csrc/kernels/lenet.hip k_fc1_fwd k_fc_bwd
    python tools/isa_load_order.py csrc/kernels/optim.hip k_adam k_sgd --out profiles/x.txt
    python tools/isa_load_order.py csrc/kernels/lenet_v2.hip k_conv_fwd2 --lds
    python tools/isa_load_order.py csrc/kernels/optim.hip k_adam k_sgd --scalar --lds --all-blocks
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = "gfx950"

_TOKEN = re.compile(
    r"^\s*(global_load\w*|buffer_load\w*|\w*_store\w*|\w*_atomic\w*|s_waitcnt|v_mfma\w*|s_barrier|s_cbranch\w*)\b(.*)$")
_TOKEN_LDS = re.compile(
    r"^\s*(global_load\w*|buffer_load\w*|\w*_store\w*|\w*_atomic\w*|s_waitcnt|v_mfma\w*|s_barrier|s_cbranch\w*"
    r"|ds_\w+|v_\w+_dpp)\b(.*)$")
_TOKEN_SCALAR = re.compile(r"^\s*(s_load_\w+)\b(.*)$")
_LABEL = re.compile(r"^([.\w$]+):")
_REMARK = re.compile(r"remark:\s+(.+?): (\S+)(?: \[-Rpass[^\]]*\])?\s*$")
_KEYS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]",
         "TotalSGPRs")


def file_flags(src):
    """The per-source extra flags of the real build, so the listing is the shipped code."""
    sys.path.insert(0, ROOT)
    try:
        from pytorch_distributed_example_amd.utils.build import _FILE_FLAGS
        return list(_FILE_FLAGS.get(os.path.basename(src), []))
    except Exception:
        return []


def compile_to_asm(src, extra):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = ["hipcc", "-x", "hip", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-munsafe-fp-atomics",
               "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-I" + os.path.join(ROOT, "csrc", "include")] + extra + [src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"compile failed:\n{' '.join(cmd)}\n{r.stderr}")
        with open(out) as f:
            return f.read(), r.stderr


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except Exception:
        return {n: n for n in names}


def resources(remarks):
    """{mangled name: {key: value}} from the kernel-resource-usage remarks."""
    res, cur = {}, None
    for line in remarks.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k == "Function Name":
            cur = res.setdefault(v, {})
        elif cur is not None:
            cur[k] = v
    return res


def classify_lds(op, rest, lds=True):
    """Tokens of one instruction with --lds / --scalar: the plain token (if any), lgkmcnt waits and,
    with ``lds``, the LDS-side ones."""
    if op.startswith("s_load_"):
        return ["s"]
    if op == "s_waitcnt":
        toks = []
        m = re.search(r"vmcnt\((\d+)\)", rest)
        if m:
            toks.append(f"w{m.group(1)}")
        m = re.search(r"lgkmcnt\((\d+)\)", rest)
        if m:
            toks.append(f"g{m.group(1)}")
        return toks
    if op.endswith("_dpp"):
        return ["x"] if lds else []
    if op.startswith("ds_"):
        if not lds:
            return []
        if re.match(r"ds_(bpermute|permute|swizzle)", op):
            return ["x"]
        if re.match(r"ds_(read|load)", op):
            return ["r"]
        if re.match(r"ds_(write|store)", op):
            return ["d"]
        return []                                    # LDS atomics, ds_nop, gws: not listed
    t = classify(op, rest)
    return [t] if t else []


def classify(op, rest):
    if op == "s_waitcnt":
        m = re.search(r"vmcnt\((\d+)\)", rest)
        return f"w{m.group(1)}" if m else None       # lgkmcnt-only waits are not global-memory waits
    if op.startswith("v_mfma"):
        return "M"
    if op == "s_barrier":
        return "BAR"
    if op.startswith("s_cbranch"):
        return "br"
    if "_atomic" in op:
        return "A" if op.startswith(("global_", "buffer_", "flat_")) else None
    if "_store" in op:
        return "S" if op.startswith(("global_", "buffer_", "flat_", "scratch_")) else None
    return "L"


def kernel_bodies(asm):
    """{mangled name: [lines]} for every .globl function of the assembly."""
    bodies, cur, name = {}, None, None
    for line in asm.splitlines():
        m = _LABEL.match(line)
        if m and not m.group(1).startswith("."):
            name, cur = m.group(1), []
            bodies[name] = cur
            continue
        if cur is not None:
            if line.strip().startswith(".end_amdhsa_kernel") or line.strip().startswith(".Lfunc_end"):
                cur = None
                continue
            cur.append(line)
    return bodies


def rle(tokens):
    out, i = [], 0
    while i < len(tokens):
        j = i
        while j < len(tokens) and tokens[j] == tokens[i]:
            j += 1
        n = j - i
        out.append(f"{n}{tokens[i]}" if n > 1 or tokens[i] in ("L", "S", "M", "A", "r", "d", "x", "s") else tokens[i])
        i = j
    return " ".join(out)


def order(lines, all_blocks=False, lds=False, scalar=False):
    """[(block label, rle string)] for the basic blocks that hold any matched instruction."""
    blocks, label, toks = [], "entry", []

    def keep(toks):
        return bool(toks) and (all_blocks or any(t != "br" for t in toks))

    for line in lines:
        m = _LABEL.match(line)
        if m:
            if keep(toks):
                blocks.append((label, rle(toks)))
            label, toks = m.group(1), []
            continue
        m = (_TOKEN_SCALAR.match(line) if scalar else None) or (_TOKEN_LDS if lds or scalar else _TOKEN).match(line)
        if m:
            if lds or scalar:
                toks.extend(classify_lds(m.group(1), m.group(2), lds))
            else:
                t = classify(m.group(1), m.group(2))
                if t:
                    toks.append(t)
    if keep(toks):
        blocks.append((label, rle(toks)))
    return blocks


def report(src, wanted, extra=(), all_blocks=False, lds=False, scalar=False):
    asm, remarks = compile_to_asm(src, file_flags(src) + list(extra))
    res = resources(remarks)
    bodies = kernel_bodies(asm)
    names = [n for n in bodies if n in res]
    pretty = demangle(names)
    out = []
    for n in names:
        if wanted and not any(w in pretty[n] for w in wanted):
            continue
        out.append(f"== {pretty[n]}")
        out.append("   " + "  ".join(f"{k.split(' [')[0]}={res[n].get(k, '?')}" for k in _KEYS))
        for label, seq in order(bodies[n], all_blocks, lds, scalar):
            out.append(f"   {label:>10}: {seq}")
        out.append("")
    if not out:
        raise SystemExit(f"no kernel of {src} matches {wanted}")
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="a .hip file")
    ap.add_argument("kernels", nargs="*", help="substrings of demangled kernel names (default: all)")
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("-X", dest="extra", action="append", default=[], help="extra compiler flag")
    ap.add_argument("--all-blocks", action="store_true", help="also list blocks that hold only branches")
    ap.add_argument("--lds", action="store_true",
                    help="also list LDS reads (r), writes (d), lane exchanges (x) and lgkmcnt waits (g<n>)")
    ap.add_argument("--scalar", action="store_true",
                    help="also list scalar loads (s) and lgkmcnt waits (g<n>)")
    ap.add_argument("-q", "--quiet", action="store_true", help="with --out: do not print the report")
    a = ap.parse_args(argv)
    text = report(a.source, a.kernels, a.extra, a.all_blocks, a.lds, a.scalar)
    if not (a.quiet and a.out):
        print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
