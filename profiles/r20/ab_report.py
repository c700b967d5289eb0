#!/usr/bin/env python3
"""ab_summary.txt from the round files put next to it (the tools' own output; not kept in the repository): e2e_round<r>_{parent,change}.json (tools/e2e_bench.py --modes
malloc,arena,device --repeat 4 --no-pcie) and bench_round<r>_{parent,change}.json (bench.py --full --no-cpu-baseline
--no-configs), the parent's library against the change's through JPEGBLK_LIB, four rounds in one call each, the parent
first in rounds 1 and 3, the change first in rounds 2 and 4.  Criterion per line: the change's median lies within the
parent's own round-to-round spread (max - min of its rounds) around the parent's median."""
import glob
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def e2e_figures(path):
    d = json.load(open(path))
    return {"e2e_bench %s, %d threads (images/s)" % (x["output"].split(" ")[0], x["threads"]): x["images_per_s"] for x in d["decode_path"]}


def bench_figures(path):
    line = [ln for ln in open(path).read().split("\n") if ln.startswith("{")][-1]
    d = json.loads(line)
    out = {"bench.py headline (%s)" % d.get("unit", "value"): d["value"]} if "value" in d else {}

    def walk(node, name):
        if isinstance(node, dict):
            for k, v in node.items():
                if k == "images_per_s" and isinstance(v, (int, float)):
                    out["bench.py end_to_end %s (images/s)" % name] = v
                else:
                    walk(v, (name + " " + k).strip())
    walk(d.get("end_to_end", {}).get("runs", {}), "")
    return out


def main():
    rows, within, total = [], 0, 0
    for prefix, figures in (("e2e", e2e_figures), ("bench", bench_figures)):
        rounds = sorted({int(os.path.basename(p).split("_")[1][5:]) for p in glob.glob(os.path.join(HERE, prefix + "_round*_parent.json"))})
        if not rounds:
            continue
        sides = {s: [figures(os.path.join(HERE, "%s_round%d_%s.json" % (prefix, r, s))) for r in rounds] for s in ("parent", "change")}
        for key in sides["parent"][0]:
            p = [f[key] for f in sides["parent"]]
            c = [f[key] for f in sides["change"]]
            mp, mc, spread = statistics.median(p), statistics.median(c), max(p) - min(p)
            ok = abs(mc - mp) <= spread
            within, total = within + ok, total + 1
            rows.append("%s\n  parent %s  median %.6g  spread %.6g (%.2f %%)\n  change %s  median %.6g  d %+.2f %%  %s" %
                        (key, p, mp, spread, 100 * spread / mp, c, mc, 100 * (mc - mp) / mp, "within" if ok else "OUTSIDE"))
    head = __doc__.split('"""')[0].strip() + "\n\n"
    text = head + "\n".join(rows) + "\n\n%d of %d lines within the parent's spread.\n" % (within, total)
    open(os.path.join(HERE, "ab_summary.txt"), "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
