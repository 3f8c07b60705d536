#!/usr/bin/env python3
"""VGPRs, SGPRs, LDS, spilled dwords and scratch bytes of a source's kernels (compiles it to ISA text).  By default every
k_eval_forest instantiation of rdf_hip.hip.
usage: python3 tools/kernel_regs.py [--src FILE.hip of 3d-beats_amd/csrc] [--kernel NAME-PREFIX] [substring of the demangled name]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-beats_amd", "csrc")


def main(filt="", src="rdf_hip.hip", kernel="k_eval_forest"):
    d = tempfile.mkdtemp(prefix="rdf_isa_")
    stem = os.path.splitext(os.path.basename(src))[0]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-fast-math", "-ffp-contract=off",
                           "--save-temps", "-c", "-o", os.path.join(d, "rdf.o"), os.path.join(CSRC, src)], cwd=d, stderr=subprocess.DEVNULL)
    s = open(os.path.join(d, stem + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    md = s[s.find("amdhsa.kernels"):]
    for b in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        if kernel not in name:
            continue
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        short = dem[dem.find(kernel):]
        short = short[:short.find(">(") + 1] if ">(" in short else short.split("(")[0]
        if filt not in short:
            continue
        i = s.find("\n" + name + ":")
        body = s[i:s.find(".end_amdhsa_kernel", i)]
        def field(key):
            return re.search(key + r":\s+(\d+)", b).group(1)
        print(f"{short:62s} vgpr {field('.vgpr_count'):>3s} sgpr {field('.sgpr_count'):>3s} lds {field('.group_segment_fixed_size'):>5s} B "
              f"spill {field('.vgpr_spill_count'):>3s} scratch {field('.private_segment_fixed_size'):>4s} B  lines {body.count(chr(10)):5d}")


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {}
    for flag, key in (("--src", "src"), ("--kernel", "kernel")):
        if flag in args:
            at = args.index(flag)
            opts[key] = args[at + 1]
            del args[at:at + 2]
    main(args[0] if args else "", **opts)
