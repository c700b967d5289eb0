"""What profiles/r19/resources_tile_kernels.txt and front_end_intervals.txt were made with: two builds of
jpeg_decoder_amd/csrc/jb_kernels.hip (hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --save-temps
-Rpass-analysis=kernel-resource-usage, stderr kept), the parent's and the change's, side by side.

  python profiles/r19/front_end_report.py resources <parent remarks> <change remarks>
  python profiles/r19/front_end_report.py intervals <parent .s> <change .s>

resources: every jb_tile_kernel instantiation's VGPRs, SGPRs, waves per SIMD, scratch and spills, and a verdict line.
intervals: for jb_tile_kernel<1, 1, false, false> (the headline: 4:4:4, row-bound, interleaved u8), the instructions
from the kernel's label to its first LDS-DMA load, from the first to the last of them on the full-tile path, and from the
wait for the coefficients to the first dequantising multiply, with the scalar table loads of that last interval."""
import re
import subprocess
import sys

OCC, SCR = "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]"
HEADLINE = "_Z14jb_tile_kernelILi1ELi1ELb0ELb0ELb0ELi1ELi0ELi0EJEEv8JbLaunchDpKT7_"


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return {k: v for k, v in out.items() if "jb_tile_kernel" in k}


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, (s.replace("void ", "").split("(")[0] for s in r.stdout.splitlines())))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def cmd_resources(parent, change):
    a, b = resources(parent), resources(change)
    pretty = demangle(sorted(a))
    worse = []
    print(f"{'instantiation':78s} {'VGPR':>9s} {'SGPR':>9s} {'waves':>7s} {'scratch':>9s} {'spills':>7s}   (parent -> change)")
    for k in sorted(a):
        x, y = a[k], b[k]
        sp = lambda r: r["SGPRs Spill"] + r["VGPRs Spill"]
        print(f"{pretty[k]:78s} {x['VGPRs']:4d}->{y['VGPRs']:<4d} {x['TotalSGPRs']:4d}->{y['TotalSGPRs']:<4d} {x[OCC]:3d}->{y[OCC]:<3d} "
              f"{x[SCR]:4d}->{y[SCR]:<4d} {sp(x):3d}->{sp(y):<3d}")
        if y[OCC] < x[OCC] or y[SCR] > x[SCR] or sp(y) > sp(x):
            worse.append(pretty[k])
    print(f"\n{len(a)} instantiations; a wave per SIMD lost or scratch gained: {worse if worse else 'none'}")
    assert sorted(a) == sorted(b), "the two builds instantiate different kernels"


def body(path, label):
    lines = open(path).read().split("\n")
    i = lines.index(next(l for l in lines if l.startswith(label + ":")))
    out = []
    for l in lines[i + 1:]:
        s = l.strip()
        if s.startswith("s_endpgm"):
            break
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        out.append(s)
    return out


def intervals(path):
    ins = body(path, HEADLINE)
    loads = [i for i, s in enumerate(ins) if s.startswith("global_load_lds_dwordx4")]
    # the eight loads a full tile issues: the only eight of the parent; where the ragged tile has a path of its own,
    # the densest run of eight (the ragged path's clamps make it the longer one wherever hipcc puts it)
    # (hipcc lays the ragged path out first and a full tile branches over it: its instructions are not executed, so they
    # are taken out before counting)
    assert len(loads) in (8, 16), "one path, or a full-tile and a ragged path of eight loads each"
    n_loads = len(loads)
    if len(loads) == 16:
        dense = min((0, 8), key=lambda k: loads[k + 7] - loads[k])
        assert dense == 8, "expected the ragged path in front of the full-tile path"
        branch = max(i for i in range(loads[0]) if ins[i].startswith("s_cbranch"))
        ins = ins[:branch + 1] + ins[loads[7] + 1:]
        loads = [i for i, s in enumerate(ins) if s.startswith("global_load_lds_dwordx4")]
    first, last = loads[0], loads[7]
    wait = next(i for i in range(last, len(ins)) if ins[i].startswith("s_waitcnt vmcnt(0)"))
    mul = next(i for i in range(wait, len(ins)) if ins[i].startswith("v_mul_i32_i24"))
    sl = [s for s in ins[wait:mul] if s.startswith("s_load_dword")]
    valu = sum(1 for s in ins[first:last] if s.startswith("v_"))
    return first, last - first - 7, valu, mul - wait - 1, sl, sum(1 for s in ins[:first] if s.startswith("s_load_dword")), n_loads


def cmd_intervals(parent, change):
    for tag, path in (("parent", parent), ("change", change)):
        a, b, valu, c, sl, pre, n = intervals(path)
        print(f"{tag}: label -> first global_load_lds: {a} instructions ({pre} of them the scalar loads of arguments and table)")
        print(f"{tag}: first -> eighth global_load_lds, the loads themselves not counted: {b} instructions, {valu} of them VALU ({n} LDS-DMA loads in the kernel; of 16, the ragged tile's eight are branched over and not counted)")
        print(f"{tag}: s_waitcnt vmcnt(0) -> first v_mul_i32_i24: {c} instructions, scalar table loads among them: {len(sl)}")
        for s in sl:
            print(f"{tag}:     {s}")


if __name__ == "__main__":
    {"resources": cmd_resources, "intervals": cmd_intervals}[sys.argv[1]](sys.argv[2], sys.argv[3])
