#!/usr/bin/env python3
"""Record the host front end's verdicts on the files of tests/frontend_cases.py; no device is needed:
    python tools/record_frontend_verdicts.py [--csrc DIR] [--source TEXT] [out.json]   (default: tests/golden/frontend_verdicts.json)
--csrc DIR builds tools/fuzz/frontend_verdicts.cpp against the front end's sources in DIR (another commit's
jpeg_decoder_amd/csrc) instead of this tree's; --source says in the file's header where they came from.

The file holds every distinct field of a row once ("fields": "status|text|what came back"), the structured cases and
the entry points' rows in full as lists of indices into that table, one per call of the row, and every sweep as the
number of its rows, the SHA-256 over them and the number of distinct (status, text) outcomes in them.  "texts" are the
message texts of set_err(...) and done(...) in the two front-end sources that were recorded.  To find out which row of a
sweep differs, run this script on both trees with --rows and diff what it prints."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "frontend_verdicts.json")
CSRC = os.path.join(ROOT, "jpeg_decoder_amd", "csrc")
FUZZ = os.path.join(ROOT, "tools", "fuzz")
SOURCES = ("jb_frontend.cpp", "jb_frontend_ext.cpp", "jb_geometry.cpp", "jb_exif.cpp", "jb_huff_pack.cpp", "jb_hostutil.cpp")


def build(csrc=None, directory=None):
    """-> (the program, None) or (None, the build's error text).  This tree's: tools/fuzz/Makefile; another csrc: the
    same command line, into `directory`."""
    if csrc is None:
        b = subprocess.run(["make", "-C", FUZZ, "frontend_verdicts"], capture_output=True, text=True)
        return (os.path.join(FUZZ, "frontend_verdicts"), None) if b.returncode == 0 else (None, b.stderr)
    exe = os.path.join(directory, "frontend_verdicts")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-pthread", "-I" + csrc, "-o", exe, os.path.join(FUZZ, "frontend_verdicts.cpp")] +
                       [os.path.join(csrc, s) for s in SOURCES], capture_output=True, text=True, cwd=FUZZ)
    return (exe, None) if b.returncode == 0 else (None, b.stderr)


def texts_of(csrc):
    """The message texts of set_err(...) and done(...) in the two front-end sources (and the headers they keep them in)."""
    found = set()
    for name in ("jb_frontend.cpp", "jb_frontend_ext.cpp", "jb_markers.h"):
        path = os.path.join(csrc, name)
        if os.path.exists(path):
            with open(path) as fh:
                src = fh.read()
            found |= set(re.findall(r'\b(?:set_err|done)\(\s*\w+\s*,\s*[\w:]+\s*,\s*"([^"]+)"', src))
            found |= set(re.findall(r'\bdone\(\s*[\w:]+\s*,\s*"([^"]+)"', src))
    return sorted(found)


def rows_of(exe):
    """Runs the program over the cases -> ([(name, [field, ...])] in the program's order, structured names, sweeps)."""
    import frontend_cases
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.txt")
        structured, sweeps = frontend_cases.cases_file(path)
        good, corrupt = frontend_cases.entry_files(d)
        # the cases are independent: every n-th of them to one of n processes, the entry points' rows with the last
        with open(path) as fh:
            lines = fh.read().split("\n")
        seeds, cases = [x for x in lines if x.startswith("S\t")], [x for x in lines if x and not x.startswith("S\t")]
        n = max(1, min(16, len(os.sched_getaffinity(0))))
        procs = []
        for i in range(n):
            share = os.path.join(d, "cases%d.txt" % i)
            with open(share, "w") as fh:
                fh.write("\n".join(seeds + cases[i::n]) + "\n")
            with open(share + ".out", "w") as so, open(share + ".err", "w") as se:  # (files: a full pipe would stall a process)
                procs.append(subprocess.Popen([exe, share] + ([good, corrupt] if i == n - 1 else ["-", "-"]), stdout=so, stderr=se))
        outs = []
        for i, p in enumerate(procs):
            p.wait(timeout=900)
            with open(os.path.join(d, "cases%d.txt.out" % i)) as so, open(os.path.join(d, "cases%d.txt.err" % i)) as se:
                outs.append((so.read(), se.read()))
            if p.returncode != 0:
                raise RuntimeError("frontend_verdicts failed:\n" + (outs[-1][0][-1500:] + outs[-1][1][-3000:]))
    rows = []
    for so, _ in outs:
        for line in so.split("\n"):
            if line:
                name, *fields = line.split("\t")
                rows.append((name, [f.split("=", 1)[1] if not name.startswith("entry:") else f for f in fields]))
    order = {x.split("\t")[1]: i for i, x in enumerate(cases)}
    rows.sort(key=lambda r: order.get(r[0], len(order)))  # (stable: the entry points' rows stay in their order, last)
    return rows, structured, sweeps


def table_of(rows, structured, sweeps):
    """-> the dictionary the golden file holds (without its header)."""
    by_name = dict(rows)
    assert len(by_name) == len(rows), "case names are not distinct"
    entries = [name for name, _ in rows if name.startswith("entry:")]
    assert sorted(by_name) == sorted(structured + entries + [n for names in sweeps.values() for n in names])
    fields = sorted({f for name in structured + entries for f in by_name[name]})
    index = {f: i for i, f in enumerate(fields)}
    out = {"fields": fields,
           "cases": {name: [index[f] for f in by_name[name]] for name in structured},
           "entries": {name: [index[f] for f in by_name[name]] for name in entries},
           "sweeps": {}}
    for sweep, names in sweeps.items():
        h = hashlib.sha256()
        outcomes = set()
        for name in names:
            h.update((name + "\t" + "\t".join(by_name[name]) + "\n").encode())
            outcomes |= {tuple(f.split("|")[:2]) for f in by_name[name] if "|" in f}
        out["sweeps"][sweep] = {"rows": len(names), "sha256": h.hexdigest(), "outcomes": len(outcomes)}
    return out


def dump(header, table, path):
    lines = lambda d: ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in d.items())
    with open(path, "w") as fh:
        fh.write('{"header": %s,\n"texts": %s,\n"fields": [\n%s\n],\n"cases": {\n%s\n},\n"entries": {\n%s\n},\n"sweeps": {\n%s\n}}\n' %
                 (json.dumps(header), json.dumps(header.pop("texts")), ",\n".join(json.dumps(f) for f in table["fields"]),
                  lines(table["cases"]), lines(table["entries"]), lines(table["sweeps"])))


def load(path=GOLDEN):
    """-> the file with "cases" and "entries" as {name: [field, ...]}."""
    with open(path) as fh:
        t = json.load(fh)
    for key in ("cases", "entries"):
        t[key] = {name: [t["fields"][i] for i in row] for name, row in t[key].items()}
    return t


def main():
    args = sys.argv[1:]
    csrc = source = None
    show_rows = "--rows" in args
    if show_rows:
        args.remove("--rows")
    while args and args[0] in ("--csrc", "--source"):
        if args[0] == "--csrc":
            csrc = os.path.abspath(args[1])
        else:
            source = args[1]
        args = args[2:]
    out = args[0] if args else GOLDEN
    with tempfile.TemporaryDirectory() as d:
        exe, err = build(csrc, d)
        if exe is None:
            sys.exit(err)
        rows, structured, sweeps = rows_of(exe)
    if show_rows:
        for name, fields in rows:
            print(name + "\t" + "\t".join(fields))
        return
    table = table_of(rows, structured, sweeps)
    if source is None:  # (recording anew with this tree's sources keeps the header: the file must come out byte for byte)
        with open(GOLDEN) as fh:
            old = json.load(fh)
        header = dict(old["header"], texts=old["texts"])
    else:
        header = {"recorded_from": source, "by": "tools/record_frontend_verdicts.py", "texts": texts_of(csrc or CSRC)}
    dump(header, table, out)
    print(f"{len(structured)} structured cases, {len(table['entries'])} entry-point rows, {len(sweeps)} sweeps of "
          f"{sum(len(v) for v in sweeps.values())} rows, {len(table['fields'])} distinct fields, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()
