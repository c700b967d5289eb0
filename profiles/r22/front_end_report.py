"""What profiles/r22/resources_tile_kernels.txt and front_end_intervals.txt were made with, on top of
profiles/r19/front_end_report.py (the same two builds of jpeg_decoder_amd/csrc/jb_kernels.hip: hipcc --offload-arch=gfx950
-O3 -std=c++17 -fPIC -ffp-contract=off --save-temps -Rpass-analysis=kernel-resource-usage, the change's also with
-mllvm -amdgpu-kernarg-preload-count=1 as csrc/Makefile builds it; stderr kept as the remarks).

  python profiles/r22/front_end_report.py resources <parent remarks> <change remarks> <parent .s> <change .s>
  python profiles/r22/front_end_report.py intervals <parent .s> <change .s>

resources: r19's table for the instantiations both builds have, the new entries' own rows, whether each common
instantiation's instruction stream is the parent's (labels renumbered): identical, the same opcodes in the same order with
operands that differ, or different, and every kernel's
.amdhsa_user_sgpr_kernarg_preload_length.
intervals: r19's three intervals for jb_tile_kernel<1, 1, false, false> of both builds, and for the change's flat entry
jb_tile_kernel_flat<false, 0>: from the instruction the hardware starts at when it has preloaded (behind the
compatibility prologue, which ends with the first s_branch) to the first LDS-DMA load, with the s_waitcnt lgkmcnt
instructions in front of that load counted -- there must be none."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "r19"))
import front_end_report as r19  # noqa: E402

FLAT = "_Z19jb_tile_kernel_flatILb0ELi0EJEEvPKh8JbLaunchDpKT1_"


def stream(path, label):
    """the kernel's instructions with its local labels renumbered in order of appearance"""
    names = {}
    out = []
    for s in r19.body(path, label):
        s = re.sub(r"\s*;.*$", "", s)
        out.append(re.sub(r"\.LBB\d+_\d+", lambda m: names.setdefault(m.group(0), f".L{len(names)}"), s))
    return out


def preload_lengths(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", line)
        if m and name:
            out[name] = int(m.group(1))
    return out


def cmd_resources(parent_r, change_r, parent_s, change_s):
    a, b = r19.resources(parent_r), r19.resources(change_r)
    new = sorted(set(b) - set(a))
    assert not set(a) - set(b), "an instantiation of the parent is gone"
    pretty = r19.demangle(sorted(b))
    sp = lambda r: r["SGPRs Spill"] + r["VGPRs Spill"]
    worse, differ = [], []
    print(f"{'instantiation':78s} {'VGPR':>9s} {'SGPR':>9s} {'waves':>7s} {'scratch':>9s} {'spills':>7s}  instructions   (parent -> change)")
    for k in sorted(a):
        x, y = a[k], b[k]
        sa, sb = stream(parent_s, k), stream(change_s, k)
        same = sa == sb
        # not the same text: the same opcodes in the same order (operands of commutative instructions swapped), or not even that
        verdict = "identical" if same else (f"same opcodes, {sum(x_ != y_ for x_, y_ in zip(sa, sb))} lines differ in operands"
                                            if [t.split()[0] for t in sa] == [t.split()[0] for t in sb] else "DIFFERENT")
        print(f"{pretty[k]:78s} {x['VGPRs']:4d}->{y['VGPRs']:<4d} {x['TotalSGPRs']:4d}->{y['TotalSGPRs']:<4d} {x[r19.OCC]:3d}->{y[r19.OCC]:<3d} "
              f"{x[r19.SCR]:4d}->{y[r19.SCR]:<4d} {sp(x):3d}->{sp(y):<3d}  {len(sa):5d} {verdict}")
        if y[r19.OCC] < x[r19.OCC] or y[r19.SCR] > x[r19.SCR] or sp(y) > sp(x):
            worse.append(pretty[k])
        if verdict == "DIFFERENT":
            differ.append(pretty[k])
    print("\nnew entries (change only):")
    for k in new:
        y = b[k]
        print(f"{pretty[k]:78s} VGPR {y['VGPRs']}  SGPR {y['TotalSGPRs']}  waves {y[r19.OCC]}  scratch {y[r19.SCR]}  spills {sp(y)}  {len(stream(change_s, k))} instructions")
    print(f"\n{len(a)} common instantiations; a wave per SIMD lost or scratch gained: {worse if worse else 'none'}; "
          f"opcode sequence not the parent's: {differ if differ else 'none'}")
    pl = preload_lengths(change_s)
    nz = {k: v for k, v in pl.items() if v}
    print(f"kernel-argument preload length of the change's {len(pl)} kernels (every kernel of jb_kernels.hip): non-zero for {len(nz)}:")
    for k, v in sorted(nz.items()):
        print(f"    {v} SGPRs  {r19.demangle([k])[k]}")
    assert all(v == 0 for v in preload_lengths(parent_s).values())


def flat_intervals(path):
    ins = r19.body(path, FLAT)
    start = next(i for i, s in enumerate(ins) if s.startswith("s_branch")) + 1  # the compatibility prologue ends here
    ins = ins[start:]
    loads = [i for i, s in enumerate(ins) if s.startswith("global_load_lds_dwordx4")]
    assert len(loads) == 8, "the flat entry has the full tile's eight loads and no ragged path"
    first, last = loads[0], loads[7]
    waits = [s for s in ins[:first] if s.startswith("s_waitcnt") and "lgkmcnt" in s]
    sl = sum(1 for s in ins[:first] if s.startswith("s_load_dword"))
    wait = next(i for i in range(last, len(ins)) if ins[i].startswith("s_waitcnt lgkmcnt(0)"))
    return start, first, last - first - 7, sum(1 for s in ins[first:last] if s.startswith("v_")), waits, sl, wait - last - 1


def cmd_intervals(parent, change):
    r19.cmd_intervals(parent, change)
    pro, a, b, valu, waits, sl, c = flat_intervals(change)
    print(f"change, flat entry: compatibility prologue (skipped where the firmware preloads): {pro} instructions")
    print(f"change, flat entry: entry -> first global_load_lds: {a} instructions ({sl} of them scalar loads of the structure, issued and not waited for); "
          f"s_waitcnt lgkmcnt among them: {len(waits)}")
    print(f"change, flat entry: first -> eighth global_load_lds, the loads themselves not counted: {b} instructions, {valu} of them VALU (8 LDS-DMA loads in the kernel)")
    print(f"change, flat entry: eighth global_load_lds -> the first s_waitcnt lgkmcnt(0), the wait for the structure: {c} instructions")
    assert not waits, "a wait for scalar memory stands in front of the flat entry's first load"


if __name__ == "__main__":
    {"resources": cmd_resources, "intervals": cmd_intervals}[sys.argv[1]](*sys.argv[2:])
