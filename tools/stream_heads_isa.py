#!/usr/bin/env python3
"""Does the compiler still emit the heads of the sliced streaming kernels the way lsq_sell.h needs them?

The gain of the LDS-DMA heads (k_sell_cols, k_sell_rows with an unscaled gather vector; docs/LABNOTES.md, "Sliced products: the
head of a streaming launch") rests on three properties of the generated code that no test of results can see, because a kernel
that lost them computes the same bits, only slower:
  1. no spilled register and no scratch memory in a sliced kernel (1024-thread workgroups: 128 VGPRs is the cap);
  2. the gather vector goes global -> LDS by global_load_lds_dwordx4 (no staging registers);
  3. the eight global_load_dwordx4 of a wave's first batch are issued behind the last of those copies and AHEAD of the
     s_barrier that follows, with no s_waitcnt vmcnt between the first and the last of them.
Run it after a change to lsq_sell.h / lsq_spmv.h and after a compiler update (needs hipcc, no GPU):

    python tools/stream_heads_isa.py            # or: make -C leastsquaresoptim.jl_amd/csrc check-heads

It compiles lsq_sparse.hip and lsq_model.hip for gfx950 with the Makefile's flags and --save-temps into temporary
directories, prints one line per sliced kernel they instantiate (VGPRs, spilled, scratch bytes, copies, requests of the first
batch ahead of the barrier) and exits 1 if a kernel that must have the head lacks one of the three.  What it cannot decide is left to the reader: whether a wait sits on
the path between the first copy and the batch for a launch's FIRST block (later blocks of a workgroup's block loop do wait);
`--show KERNEL` prints the loads, waits, barriers and branches of one kernel for that."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "leastsquaresoptim.jl_amd", "csrc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-result -Wno-unused-value -ffp-contract=off".split()
DMA, BATCH = "global_load_lds_dwordx4", "global_load_dwordx4"
# kernels that must have the DMA head (mangled-name fragments); the other sliced kernels are listed for their registers only
HEADS = ("11k_sell_colsILb0E", "11k_sell_colsILb1E", "11k_sell_rowsI17EpiResidualSqPerm")
LISTED = ("k_sell_",)
SOURCES = ("lsq_sparse.hip", "lsq_model.hip")        # between them every instance named in HEADS


def compile_isa(hipcc, source):
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([hipcc] + FLAGS + ["--save-temps", "-c", os.path.join(CSRC, source), "-o", "out.o"],
                       cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for name in os.listdir(tmp):
            if name.endswith(".s") and "amdgcn" in name:
                return open(os.path.join(tmp, name)).read().splitlines()
    raise SystemExit("no device assembly among the temporaries of " + source)


def metadata(lines):
    """mangled name -> {vgpr_count, vgpr_spill_count, private_segment_fixed_size} from the amdhsa.kernels notes."""
    out, cur = {}, {}
    for ln in lines:
        m = re.match(r"\s*(- )?\.(\w+):\s*(\S+)", ln)
        if not m:
            continue
        if m.group(1):                       # a new list entry; kernels are the entries that carry a .symbol
            if "symbol" in cur:
                out[cur["name"]] = cur
            cur = {}
        cur[m.group(2)] = m.group(3)
    if "symbol" in cur:
        out[cur["name"]] = cur
    return out


def body(lines, name):
    start = next(k for k, ln in enumerate(lines) if ln.startswith(name + ":"))
    end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
    return [ln.split(";")[0].strip() for ln in lines[start + 1:end]]


def head(ins):
    """(copies, requests of the first batch, a vmcnt wait among them): of the stretches between two s_barrier, the one with
    the most global_load_dwordx4 behind its last copy (the re-staging inside a block loop has copies and no batch)"""
    bars = [-1] + [k for k, s in enumerate(ins) if s.startswith("s_barrier")] + [len(ins)]
    best = (0, 0, False)
    for lo, hi in zip(bars, bars[1:]):
        copies = [k for k in range(lo + 1, hi) if ins[k].startswith(DMA)]
        if not copies:
            continue
        batch = [k for k in range(copies[-1], hi) if ins[k].startswith(BATCH + " ")]
        waits = bool(batch) and any("vmcnt" in ins[k] for k in range(batch[0], batch[-1]))
        if not best[0] or len(batch) > best[1]:
            best = (len(copies), len(batch), waits)
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--show", metavar="KERNEL", help="print the memory skeleton of the kernels whose mangled name contains this")
    ap.add_argument("--asm", metavar="FILE", nargs="+", help="read these gfx950 assembly files; compile nothing")
    a = ap.parse_args()
    files = [open(f).read().splitlines() for f in a.asm] if a.asm else [compile_isa(a.hipcc, src) for src in SOURCES]
    bad, seen = 0, set()
    print("%-72s %5s %7s %7s %6s %6s" % ("kernel", "VGPRs", "spilled", "scratch", "copies", "batch"))
    for lines, (name, md) in ((lines, item) for lines in files for item in sorted(metadata(lines).items())):
        if name in seen or not any(t in name for t in LISTED):
            continue
        seen.add(name)
        ins = body(lines, name)
        copies, batch, waits = head(ins)
        vg, sp, scr = int(md["vgpr_count"]), int(md["vgpr_spill_count"]), int(md["private_segment_fixed_size"])
        why = []
        if any(t in name for t in HEADS):
            if sp or scr:
                why.append("spills")
            if not copies:
                why.append("no LDS-DMA")
            if batch < 8:
                why.append("first batch not ahead of the barrier")
            if waits:
                why.append("a vmcnt wait inside the first batch")
        bad += bool(why)
        print("%-72s %5d %7d %7d %6d %6d %s" % (name[:72], vg, sp, scr, copies, batch, ("<-- " + ", ".join(why)) if why else ""))
        if a.show and a.show in name:
            for s in ins:
                if re.match(r"global_load|buffer_load|scratch_|s_waitcnt|s_barrier|s_cbranch|s_endpgm|\.LBB", s):
                    print("    " + s)
    missing = [t for t in HEADS if not any(t in name for name in seen)]
    if missing:
        print("not found: " + ", ".join(missing))
    return 1 if bad or missing else 0


if __name__ == "__main__":
    sys.exit(main())
