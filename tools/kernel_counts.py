"""Instruction count, VGPRs, SGPRs and static LDS of every kernel in gfx950 assembly files written by `hipcc --save-temps`
(`<name>-hip-amdgcn-amd-amdhsa-gfx950.s`), side by side for two builds of one source: the record kept when code moves between files and
the machine code must not (profiles/yaapt_long_split.txt).

    python tools/kernel_counts.py BEFORE.s AFTER.s [EXTRA.s ...]

A kernel's instructions are the lines between its label and its `.Lfunc_end`, labels, directives and comments left out.  The last column
says whether the two instruction streams are the same text (branch labels and all)."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    meta = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        g = lambda key: int(re.search(r"\.amdhsa_" + key + r" (\d+)", body).group(1))
        meta[name] = dict(lds=g("group_segment_fixed_size"))
    for name in meta:
        # the code: from the label to the kernel descriptor's section (the descriptor follows the last instruction)
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\s*\.section\s+\.rodata", text, flags=re.S | re.M)
        lines = [l.split(";")[0].strip() for l in m.group(1).split("\n")]
        ins = [l for l in lines if l and not l.startswith(".") and not l.endswith(":")]
        v = re.search(r"\.set " + re.escape(name) + r"\.num_vgpr, (\d+)", text)
        s = re.search(r"\.set " + re.escape(name) + r"\.numbered_sgpr, (\d+)", text)
        meta[name].update(n=len(ins), text="\n".join(l for l in lines if l), vgpr=int(v.group(1)), sgpr=int(s.group(1)))
    return meta


def demangle(names):
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*", "", d) for n, d in zip(names, out)}


def main(argv):
    before, after = kernels(argv[0]), kernels(argv[1])
    short = demangle(sorted(set(before) | set(after)))
    print(f"{'kernel':58s} {'instr':>13s} {'VGPR':>9s} {'SGPR':>9s} {'LDS bytes':>13s}  same text")
    for n in sorted(set(before) | set(after)):
        a, b = before.get(n), after.get(n)
        col = lambda k: f"{a[k] if a else '-'} -> {b[k] if b else '-'}"
        same = "yes" if a and b and a["text"] == b["text"] else "NO"
        print(f"{short[n]:58s} {col('n'):>13s} {col('vgpr'):>9s} {col('sgpr'):>9s} {col('lds'):>13s}  {same}")
    for extra in argv[2:]:
        ks = kernels(extra)
        short = demangle(sorted(ks))
        print(f"\n{extra.split('/')[-1]}")
        for n in sorted(ks):
            k = ks[n]
            print(f"{short[n]:58s} {k['n']:>13d} {k['vgpr']:>9d} {k['sgpr']:>9d} {k['lds']:>13d}")


if __name__ == "__main__":
    main(sys.argv[1:])
