"""Do two trees compile to the same device code?  Compares, kernel by kernel, the
hipcc -S --cuda-device-only listings (`make isa OBJDIR=<dir>` in csrc/) of two
builds: the text from the `_Z...:` label to `.Lfunc_end` (instructions and the
.amdhsa_kernel descriptor) plus the kernel's amdhsa.kernels metadata entry.
    python tools/isa_same.py <dir_a> <dir_b> [old=new | mapfile ...]
`old=new` (or a file of such lines) renames a symbol of <dir_a>, for a kernel
whose template parameter list changed.  Text only: the source hash
(__hip_cuid_*), the per-function numbering of local labels and the comdat
section of a template instantiation (a kernel that stopped being a template
returns to plain .text) are blanked.
Exit status 1 if any kernel present in both differs."""
import glob
import os
import re
import sys


def kernels(d, renames):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        t = open(path).read()
        for old, new in renames:
            t = t.replace(old, new)
        t = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", t)
        t = re.sub(r"(\.L|\b)(BB|func_begin|func_end|tmp|JTI)\d+", r"\1\2", t)
        t = re.sub(r'\.section\t\.text\.\S+,"axG",@progbits,\S+,comdat', ".text", t)
        t = re.sub(r"[ \t]+;", " ;", t)   # comment columns move with a label's width
        meta = t[t.find("amdhsa.kernels:"):]
        meta = meta[:meta.find("\namdhsa.", 1)]
        ents = {re.search(r"\.name:\s+(\S+)", e).group(1): e for e in re.split(r"\n  - ", meta)[1:]}
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end", t, re.M | re.S):
            out[m.group(1)] = (os.path.basename(path), m.group(0) + ents.get(m.group(1), ""))
    return out


def main():
    pairs = []
    for a in sys.argv[3:]:
        pairs += open(a).read().split() if os.path.exists(a) else [a]
    renames = [p.split("=", 1) for p in pairs]
    a, b = kernels(sys.argv[1], renames), kernels(sys.argv[2], [])
    renamed = {new for _, new in renames}
    n = dict.fromkeys(("identical", "renamed and identical", "different", "only in first", "only in second"), 0)
    for k in sorted(set(a) | set(b)):
        if k in a and k in b:
            same = a[k][1] == b[k][1]
            what = "different" if not same else "renamed and identical" if k in renamed else "identical"
        else:
            what = "only in first" if k in a else "only in second"
        n[what] += 1
        print(f"{what:22s} {(a.get(k) or b[k])[0]:24s} {k}")
    print(", ".join(f"{v} {k}" for k, v in n.items()))
    sys.exit(1 if n["different"] else 0)


if __name__ == "__main__":
    main()
