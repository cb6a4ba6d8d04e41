"""Compare the device code of two builds of one translation unit, kernel by kernel.

    hipcc --offload-arch=gfx950 <the flags of sinddm_amd/build.py, without -shared> -c sinddm_bwd.hip --save-temps   (in two trees)
    python tools/asm_kernel_diff.py OLD/sinddm_bwd-hip-amdgcn-amd-amdhsa-gfx950.s NEW/sinddm_bwd-hip-amdgcn-amd-amdhsa-gfx950.s

Per kernel it compares the instruction stream (local labels renumbered: they carry the function's index in the file) and the
.amdhsa_ kernel descriptor (register counts, scratch, LDS), and lists the kernels only one side has.  Exit status 1 if a kernel
present in both differs.
"""
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel", txt, flags=re.S | re.M):
        name = m.group(1)
        start = txt.index("\n" + name + ":")                 # the function's label ... its descriptor
        body = re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+", lambda k: ".L" + k.group(1), txt[start:m.start()])
        code = [ln.split(";")[0].rstrip() for ln in body.splitlines()]
        out[name] = ("\n".join(ln for ln in code if ln.strip()), m.group(2))
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    both = sorted(set(old) & set(new))
    bad = [k for k in both if old[k] != new[k]]
    n_ins = sum(len(old[k][0].splitlines()) for k in both)
    print(f"kernels: old {len(old)}, new {len(new)}, in both {len(both)} ({n_ins} lines of code compared)")
    print(f"identical code and descriptor: {len(both) - len(bad)}; different: {len(bad)}")
    for k in bad:
        print("  DIFFERENT", k)
    for k in sorted(set(old) - set(new)):
        print("  only in old:", k)
    for k in sorted(set(new) - set(old)):
        print("  only in new:", k)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
