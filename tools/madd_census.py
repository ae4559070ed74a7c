"""Static census of the 64-bit multiply-adds of the fused multiply at N = 4096 (tool).
    python tools/madd_census.py [--asm FILE] [-D...]
Compiles deeppowers_amd/csrc/k_ctmul_fold.hip device-only to assembly (or reads FILE, the output of an earlier such compile) and prints, for
ct_mul_quad_kernel<FoldArith, 12, 4, false, false>: the VALU and v_mad_u64_u32 counts, the multiply-adds grouped by their scalar or literal multiplier
(register-by-register products form the group "vector"), and the compiler's resource summary (registers, scratch, LDS, code size).  Counts only.
A scalar register's meaning is the build's own (the allocator names it): profiles/rNN_madd_census.txt attributes each group to its source construct."""
import collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "deeppowers_amd", "csrc", "k_ctmul_fold.hip")
KERNEL = "_ZN5dpfhe18ct_mul_quad_kernelINS_9FoldArithELi12ELi4ELb0ELb0EEE"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S"]   # csrc/Makefile HIPFLAGS


def kernel_text(lines):
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL) and l.split(":")[0].startswith(KERNEL) and not l.startswith("\t"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    tail = next(i for i in range(end, len(lines)) if "Occupancy" in lines[i])
    return lines[start + 1:end], lines[end:tail + 1]


def operands(ins):
    # v_mad_u64_u32 vdst, sdst, src0, src1, src2: register ranges hold a comma only inside brackets
    return [o.strip() for o in re.split(r",\s*(?![^\[]*\])", ins.split(None, 1)[1])]


def census(path):
    body, summary = kernel_text(open(path).read().split("\n"))
    ins = [l.split(";")[0].strip() for l in body]
    ins = [l for l in ins if l and not l.startswith(".") and not l.endswith(":")]
    valu = [l for l in ins if l.startswith("v_")]
    mads = [l for l in valu if l.startswith("v_mad_u64_u32")]
    print("ct_mul_quad_kernel<FoldArith, 12, 4, false, false>")
    print(f"  instructions {len(ins)}   VALU {len(valu)}   SALU {sum(l.startswith('s_') for l in ins)}   v_mad_u64_u32 {len(mads)}   v_lshl_add_u64 {sum(l.startswith('v_lshl_add_u64') for l in valu)}")
    groups = collections.Counter()
    by_pair = collections.defaultdict(collections.Counter)
    for m in mads:
        _, _, s0, s1, s2 = operands(m)
        scal = [s for s in (s0, s1) if not s.startswith("v")]
        regs = [s for s in scal if s.startswith("s")]
        if not scal:
            key = "vector x vector"
        elif regs:
            key = regs[0]
            other = [s for s in (s0, s1) if s != regs[0]]
            if other and not other[0].startswith("v"):
                key = f"{regs[0]} x constant"
                by_pair[key][other[0]] += 1
        else:
            key = f"literal {scal[0]}"
        groups[key + ("" if s2 != "0" else "  (addend 0)")] += 1
    print("  multiply-adds by multiplier:")
    for key, n in sorted(groups.items(), key=lambda kv: (-kv[1], kv[0])):
        print(f"    {n:5d}  {key}")
    for key, c in by_pair.items():
        print(f"  {key}, by constant: " + "  ".join(f"{k}: {n}" for k, n in sorted(c.items(), key=lambda kv: int(kv[0], 0))))
    print("  compiler summary:")
    for l in summary:
        if re.search(r"codeLenInByte|TotalNumSgprs|NumVgprs|ScratchSize|LDSByteSize|Occupancy", l) and "Total" not in l.replace("TotalNumSgprs", ""):
            print("    " + l.lstrip("; ").strip())


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--asm" in args:
        census(args[args.index("--asm") + 1])
    else:
        out = os.path.join(tempfile.mkdtemp(), "k_ctmul_fold.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + [a for a in args if a.startswith("-")] + ["-o", out, SRC])
        census(out)
