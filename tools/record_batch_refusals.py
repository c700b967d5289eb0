#!/usr/bin/env python3
"""Record the batch decoder's refusal table (tests/batch_refusal_cases.py) of the built library, on a machine with a device:
    python tools/record_batch_refusals.py [out.json]      (default: tests/golden/batch_refusals.json)
The file holds every distinct (return code, text) once ("outcomes"), every distinct list of case-name endings once ("tails":
the setters' arguments, an entry point's variants), every distinct list of outcome indices once ("answers": one index per
ending) and one line per run of consecutive cases that share the front of their name: [front, index of its tails, index of
its answers].  load() gives the rows back, one per case."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_refusals.json")


def load(path=GOLDEN):
    """-> [(case name, return code, text), ...]"""
    with open(path) as f:
        t = json.load(f)
    return [(front + ":" + tail, *t["outcomes"][i]) for front, tails, answers in t["runs"]
            for tail, i in zip(t["tails"][tails], t["answers"][answers], strict=True)]


def dump(rows, path):
    outcomes = sorted({(rc, text) for _, rc, text in rows}, key=lambda o: (-o[0], o[1]))
    index = {o: i for i, o in enumerate(outcomes)}
    runs = []   # [front, [tail, ...], [outcome index, ...]]: consecutive cases with one front
    for name, rc, text in rows:
        front, tail = name.rsplit(":", 1)
        if not runs or runs[-1][0] != front:
            runs.append([front, [], []])
        runs[-1][1].append(tail)
        runs[-1][2].append(index[(rc, text)])
    tails, answers = [], []
    for run in runs:
        for at, table in ((1, tails), (2, answers)):
            if run[at] not in table:
                table.append(run[at])
            run[at] = table.index(run[at])
    lines = lambda items: ",\n".join(json.dumps(x) for x in items)
    with open(path, "w") as f:
        f.write('{"outcomes": [\n%s\n],\n"tails": [\n%s\n],\n"answers": [\n%s\n],\n"runs": [\n%s\n]}\n' %
                (lines(list(o) for o in outcomes), lines(tails), lines(answers), lines(runs)))
    return len(outcomes), len(runs)


def main():
    import batch_refusal_cases
    import jpeg_decoder_amd as jb
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with tempfile.TemporaryDirectory() as d:
        rows = batch_refusal_cases.cases(jb, batch_refusal_cases.tiny_files(d))
    n_outcomes, n_runs = dump(rows, out)
    assert load(out) == [tuple(r) for r in rows]
    print(f"{len(rows)} rows, {n_outcomes} distinct outcomes, {n_runs} lines -> {out}")


if __name__ == "__main__":
    main()
