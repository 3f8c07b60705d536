#!/usr/bin/env python3
"""What the level loop of the forest kernel issues per level, by issue class.

tools/ubench_valu.hip measured two VALU issue rates on gfx950 with several waves per SIMD: ~2.35 cycles per wave64
instruction for v_fma_f32 / v_add_f32 / v_mul_f32 / v_add_u32 / v_mov_b32, ~4.2 cycles for everything else the kernel
uses (conversions, v_pk_*_f32, compares, v_cndmask, shifts, v_mad_u32_u24, v_perm_b32, ...).  This script compiles
rdf_hip.hip to ISA text, takes the innermost loops of one instantiation of k_eval_forest (the level loop), leaves out
the blocks of the IEEE-divide path (they run only for nodes flagged kFlagExact) and counts the instructions of each
class.  Its `half_rate_share` is tools/roofline.py's VALU_HALF_RATE_SHARE.

A kernel with plain levels (rdf_hip.hip, "plain levels") has TWO level loops of the same depth: the plain one, whose
decision is walk_step_plain (a compare and an add with carry, no leaf bit), and the general one (walk_step: the
v_and_or_b32 that sets the leaf bit tells them apart).  Both are reported, under "plain" and "general"; the top-level
figures are the general loop's, as they were before there were two.  The plain loop's `valu_level` is what ONE plain
level issues with every probe far: its blocks once each, of the LDS and the packed-table fetch (one of them runs) only
one.  (The general loop has no such figure: the marks do not catch the exact path's record fetches, so its counts hold
some blocks an ordinary level never runs; by hand its fast path is 168 VALU for four trees.)

    python3 tools/valu_mix.py [mangled-name substring, default: the packed 512-thread 4-tree kernel of the bench batch,
        k_eval_forest<512,true,4,false,4,false,1,false,false>]
        [--isa FILE   an ISA text made earlier (hipcc -S --cuda-device-only), e.g. the parent commit's]
"""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "3d-beats_amd", "csrc", "rdf_hip.hip")
FULL_RATE = {"v_fma_f32", "v_fmac_f32", "v_add_f32", "v_sub_f32", "v_subrev_f32", "v_mul_f32", "v_add_u32", "v_sub_u32",
             "v_subrev_u32", "v_mov_b32"}
# blocks of the IEEE-divide path: the divide itself, the fetch of the exact record (64-bit addressed), the mode switches
EXACT_PATH_MARKS = ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_rcp_f32", "v_lshl_add_u64", "s_setreg_imm32_b32")


def isa_text(path=None):
    if path:
        return open(path).read().splitlines()
    out = os.path.join(tempfile.gettempdir(), "rdf_hip_gfx950.s")
    newest = max(os.path.getmtime(p) for p in [SRC] + [os.path.join(os.path.dirname(SRC), h) for h in ("rdf_device.hpp", "rdf_host_state.hpp", "rdf_launch_plan.hpp")])
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-fast-math", "-ffp-contract=off",
                               "-S", "--cuda-device-only", "-o", out, SRC], stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


def norm(op):
    return op.replace("_e32", "").replace("_e64", "").replace("_sdwa", "")


def loop_counts(blocks):
    """The figures of one loop: its blocks without those of the IEEE-divide path."""
    kept = [b for b in blocks if not any(i in EXACT_PATH_MARKS for i in b["ins"])]
    count = collections.Counter(norm(i) for b in kept for i in b["ins"])
    valu = {k: v for k, v in count.items() if k.startswith("v_")}
    full = sum(v for k, v in valu.items() if k in FULL_RATE)
    half = sum(valu.values()) - full
    # one level: every block once, but only one of the two node fetches (global_load_dwordx4 / ds_read_b128 blocks)
    n_valu = lambda b: sum(1 for i in b["ins"] if i.startswith("v_"))
    fetch = [b for b in kept if any(i.startswith(("global_load_dwordx4", "ds_read_b128")) for i in b["ins"])]
    level = sum(n_valu(b) for b in kept) - (min(n_valu(b) for b in fetch) if len(fetch) == 2 else 0)
    return {"blocks_in_level_loop": len(blocks), "blocks_counted": len(kept), "valu_level": level,
            "valu_full_rate": full, "valu_half_rate": half, "half_rate_share": round(half / max(1, full + half), 3),
            "salu": sum(v for k, v in count.items() if k.startswith("s_") and not k.startswith(("s_waitcnt", "s_nop"))),
            "vmem": sum(v for k, v in count.items() if k.startswith(("global_", "buffer_", "flat_"))),
            "scratch": sum(v for k, v in count.items() if k.startswith("scratch_")),
            "lds": sum(v for k, v in count.items() if k.startswith("ds_")),
            "valu_by_opcode": dict(sorted(valu.items(), key=lambda kv: -kv[1]))}


def main(sub, isa=None):
    lines = isa_text(isa)
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and sub in l and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    body = lines[start:end]
    depth = max(int(m.group(1)) for l in body for m in [re.search(r"Depth=(\d+)", l)] if m)
    # split into basic blocks; a block's annotation says which loop it belongs to (a loop's header block says so in the
    # comment lines that follow its label)
    blocks, cur = [], None
    for l in body:
        m = re.match(r"^(\.L(BB\S+):|; %bb\.\d+:)", l)
        if m:
            cur = {"head": l, "label": m.group(2), "ins": [], "loop": None}
            blocks.append(cur)
            h = re.search(r"in Loop: Header=(BB\S+) Depth=(\d+)", l)
            if h and int(h.group(2)) == depth:
                cur["loop"] = h.group(1)
        elif cur is not None and f"Inner Loop Header: Depth={depth}" in l:
            cur["loop"] = cur["label"]
        elif cur is not None and l.startswith("\t") and not l.strip().startswith((";", ".")):
            cur["ins"].append(l.split()[0])
    loops = collections.OrderedDict()
    for b in blocks:
        if b["loop"]:
            loops.setdefault(b["loop"], []).append(b)
    # the level loops: those that hold the decision's add with carry (other loops of the same depth: staging, the pixel list)
    walks = {k: v for k, v in loops.items() if any(norm(i) == "v_addc_co_u32" for b in v for i in b["ins"])}
    general = [v for v in walks.values() if any(norm(i) == "v_and_or_b32" for b in v for i in b["ins"])]
    plain = [v for v in walks.values() if not any(norm(i) == "v_and_or_b32" for b in v for i in b["ins"])]
    out = {"kernel": lines[start].split(":")[0], "loop_depth": depth}
    out.update(loop_counts(general[0] if general else next(iter(loops.values()))))
    out.pop("valu_level")
    out["general"] = {k: v for k, v in out.items() if k not in ("kernel", "loop_depth", "valu_by_opcode")} if general else None
    out["plain"] = loop_counts(plain[0]) if plain else None
    meta = "\n".join(lines[end:end + 400])
    for key, pat in (("vgprs", r"NumVgprs: (\d+)"), ("scratch_bytes", r"ScratchSize: (\d+)"), ("occupancy", r"Occupancy: (\d+)")):
        m = re.search(pat, meta)
        out[key] = int(m.group(1)) if m else None
    out["scratch_instructions_by_loop_depth"] = scratch_by_depth(body)
    print(json.dumps(out, indent=1))


def scratch_by_depth(body):
    """Where the spills sit: scratch loads / stores per loop depth (the level loop is the deepest)."""
    d, c = 0, collections.Counter()
    for l in body:
        if re.match(r"^(\.LBB\S+:|; %bb\.\d+:)", l):
            m = re.search(r"Depth=(\d+)", l)
            d = int(m.group(1)) if m else 0
        elif l.strip().startswith("scratch_"):
            c[f"depth {d} {'load' if 'load' in l.split()[0] else 'store'}"] += 1
    return dict(sorted(c.items()))


if __name__ == "__main__":
    args = sys.argv[1:]
    isa = None
    if "--isa" in args:
        at = args.index("--isa")
        isa = args[at + 1]
        del args[at:at + 2]
    main(args[0] if args else "k_eval_forestILi512ELb1ELi4ELb0ELi4ELb0ELi1ELb0ELb0E", isa)
