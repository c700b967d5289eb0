"""The refusals of the batch decoder as one table: every case drives the public C ABI (jb_batch_decoder_*) through ctypes
and yields (case name, return code, jb_last_error text -- "" when the code is 0).  tests/golden/batch_refusals.json is this
table as tools/record_batch_refusals.py recorded it; tests/test_gpu_batch_refusals.py compares the built library with it
row by row, and tools/fuzz/batch_request_check.cpp prints the rows that need no decoder under the same names.

Names.  A decoder's request is written s<scale>a<arithmetic>o<orientation>d<draft>f<format>r<rectangle>t<target>c<fit>:
  set:<request>:<idle|busy>:<setter>(<argument>)    a setter on a decoder holding that request; busy: a batch in flight
  set:null:<setter>                                 a setter on a NULL decoder
  call:<state>:<entry point>:<variant>              an entry point (n_paths = 0 unless the variant says otherwise)
  out:<single|multi>:<case>                         arena and device regions
  collect:<case>                                    ticket errors
A NULL path is given to the submit entry points only, which check their paths; a run with n_paths = 0 has none to read.
The bad colour chain comes with one file, since a call without files has no chain to check; it is refused in every state.
No case decodes more than the four 16x16 files of tiny_files()."""
import ctypes
import itertools
import os

FMT_PLANAR = 2        # JB_FMT_RGB_F32_CHW
ORIENTS = (1, 0, 6)   # JB_ORIENT_STORED, JB_ORIENT_EXIF, a transposing code
RECT = (2, 2, 8, 8)
TARGET = (8, 8)
FIT_COVER = 2

# (setter, [(argument label, is it refused by its own argument check?), ...]) -- the order of the rows
SETTERS = (("scale", (("1", 0), ("2", 0), ("3", 1))),
           ("output_format", (("fmt0", 0), ("planar", 0), ("null", 1), ("bad", 1))),
           ("roi", (("null", 0), ("rect", 0), ("bad", 0))),
           ("resize", (("0x0", 0), ("8x8", 0), ("70000x8", 0))),
           ("filter", (("1", 0), ("99", 1))),
           ("fit", (("null", 0), ("cover", 0), ("bad", 1))),
           ("arithmetic", (("0", 0), ("1", 0), ("7", 1))),
           ("orientation", (("1", 0), ("6", 0), ("0", 0), ("9", 1))),
           ("draft", (("1", 0), ("2", 0), ("3", 1))))

CALL_STATES = ("plain", "target", "scale2", "rect", "fit", "busy", "busy2")
ENTRIES = ("", "_crops", "_views", "_views_color", "_view_groups", "_view_groups_color")


def requests():
    """every request that satisfies the invariant, over the values of the table: dicts, in a fixed order"""
    out = []
    for scale, arith, orient, draft, fmt, roi, target, fit in itertools.product((1, 2), (0, 1), ORIENTS, (1, 2), (0, FMT_PLANAR), (0, 1), (0, 1),
                                                                                (0, FIT_COVER)):
        if scale != 1 and (arith == 1 or orient != 1 or draft != 1 or fmt or roi or target):
            continue
        if draft != 1 and (arith != 1 or orient != 1):
            continue
        out.append(dict(scale=scale, arith=arith, orient=orient, draft=draft, fmt=fmt, roi=roi, target=target, fit=fit))
    return out


def request_name(q):
    return "s%da%do%dd%df%dr%dt%dc%d" % (q["scale"], q["arith"], q["orient"], q["draft"], q["fmt"], q["roi"], q["target"], q["fit"])


PLAIN = dict(scale=1, arith=0, orient=1, draft=1, fmt=0, roi=0, target=0, fit=0)
STATE_REQUESTS = {"plain": PLAIN, "target": dict(PLAIN, target=1), "scale2": dict(PLAIN, scale=2), "rect": dict(PLAIN, roi=1),
                  "fit": dict(PLAIN, target=1, fit=FIT_COVER), "busy": dict(PLAIN, target=1), "busy2": dict(PLAIN, target=1)}


def tiny_files(directory):
    """four 16x16 4:4:4 baseline files"""
    from jpeg_decoder_amd import synth
    paths = []
    for i in range(4):
        coef, q = synth.synth_blocks(16, 16, 1, 1, image_index=i)
        p = os.path.join(str(directory), "tiny%d.jpg" % i)
        with open(p, "wb") as f:
            f.write(synth.encode_jpeg(coef, 16, 16, 1, 1, q))
        paths.append(p)
    return paths


class _Driver:
    def __init__(self, jb, paths):
        self.jb, self.L, self.paths, self.rows = jb, jb.lib(), list(paths), []

    def row(self, name, rc):
        self.rows.append((name, int(rc), self.L.jb_last_error(None).decode(errors="replace") if rc else ""))
        return rc

    def create(self, multi=False):
        h = ctypes.c_void_p()
        if multi:
            rc = self.L.jb_batch_decoder_create_multi((ctypes.c_int * 2)(0, 0), 2, 2, 0, 0, ctypes.byref(h))
        else:
            rc = self.L.jb_batch_decoder_create(0, 2, 0, 0, ctypes.byref(h))
        assert rc == 0, self.L.jb_last_error(None)
        return h

    # ---- the setters -------------------------------------------------------------------------------------------------
    def setter(self, h, name, arg):
        jb, L = self.jb, self.L
        if name == "output_format":
            spec = {"fmt0": jb.OutputSpec.make(0), "planar": jb.OutputSpec.make(FMT_PLANAR), "bad": jb.OutputSpec.make(9), "null": None}[arg]
            return L.jb_batch_decoder_set_output_format(h, ctypes.byref(spec) if spec is not None else None)
        if name == "roi":
            roi = {"null": None, "rect": jb.Roi(*RECT), "bad": jb.Roi(0, 0, 0, 8)}[arg]
            return L.jb_batch_decoder_set_roi(h, ctypes.byref(roi) if roi is not None else None)
        if name == "resize":
            w, hh = arg.split("x")
            return L.jb_batch_decoder_set_resize(h, int(w), int(hh))
        if name == "fit":
            fit = {"null": None, "cover": jb.Fit.cover(), "bad": jb.Fit(9, 0, (ctypes.c_uint8 * 3)(0, 0, 0), 0, 0)}[arg]
            return L.jb_batch_decoder_set_fit(h, ctypes.byref(fit) if fit is not None else None)
        return getattr(L, "jb_batch_decoder_set_" + name)(h, int(arg))

    def establish(self, h, q):
        """the decoder's request becomes q, from whatever it was"""
        steps = [("draft", "1"), ("orientation", "1"), ("arithmetic", "0"), ("scale", "1"), ("output_format", "fmt0"), ("roi", "null"),
                 ("resize", "0x0"), ("fit", "null"), ("filter", "0"),
                 ("arithmetic", str(q["arith"])), ("orientation", str(q["orient"])), ("draft", str(q["draft"])),
                 ("output_format", "planar" if q["fmt"] else "fmt0"), ("roi", "rect" if q["roi"] else "null"),
                 ("resize", "8x8" if q["target"] else "0x0"), ("fit", "cover" if q["fit"] else "null"), ("scale", str(q["scale"]))]
        for name, arg in steps:
            rc = self.setter(h, name, arg)
            assert rc == 0, (request_name(q), name, arg, rc, self.L.jb_last_error(None))

    def batch(self, n=4):
        """the argument arrays of one call over the first n tiny files (arrays of one element at least)"""
        m = max(n, 1)
        return {"n": n, "paths": (ctypes.c_char_p * m)(*[os.fsencode(p) for p in self.paths[:n]]), "rgb": (ctypes.c_void_p * m)(),
                "w": (ctypes.c_int32 * m)(), "h": (ctypes.c_int32 * m)(), "st": (ctypes.c_int * m)(), "id": ctypes.c_int(-1)}

    def fly(self, h):
        """a batch of the four files, submitted and not collected"""
        b = self.batch()
        rc = self.L.jb_batch_decoder_submit(h, b["paths"], b["n"], b["rgb"], b["w"], b["h"], b["st"], ctypes.byref(b["id"]))
        assert rc == 0, self.L.jb_last_error(None)
        return b

    def land(self, h, b, arena=False):
        self.L.jb_batch_decoder_collect(h, b["id"], None)
        for i in range(b["n"]):
            if b["rgb"][i] and not arena:
                self.L.jb_free(b["rgb"][i])
            b["rgb"][i] = None

    def setters(self):
        h = self.create()
        for name, _ in SETTERS:
            self.row("set:null:" + name, self.setter(None, name, "1" if name not in ("output_format", "roi", "resize", "fit") else
                                                     {"output_format": "fmt0", "roi": "rect", "resize": "8x8", "fit": "cover"}[name]))
        for q in requests():
            for name, args in SETTERS:
                for arg, _ in args:
                    self.establish(h, q)
                    self.row("set:%s:idle:%s(%s)" % (request_name(q), name, arg), self.setter(h, name, arg))
            self.establish(h, q)
            b = self.fly(h)
            for name, args in SETTERS:
                for arg, _ in args:
                    rc = self.row("set:%s:busy:%s(%s)" % (request_name(q), name, arg), self.setter(h, name, arg))
                    assert rc != 0   # (else the request under the batch in flight would have changed)
            self.land(h, b)
        self.L.jb_batch_decoder_destroy(h)

    # ---- the entry points --------------------------------------------------------------------------------------------
    def variants(self, entry, submit):
        v = ["ok", "null_decoder", "null_paths", "null_rgb", "null_statuses", "negative_n"]
        if submit:
            v += ["null_ticket", "null_path"]
        if entry == "_crops":
            v += ["null_rois"]
        if entry.startswith("_views"):
            v += ["null_views", "k0", "k17"]
        if entry.startswith("_view_groups"):
            v += ["null_views", "null_groups", "n_groups0", "n_groups5", "n_views0", "reserved1"]
        if "_color" in entry:
            v += ["null_colors", "bad_chain"]
        return v

    def call(self, h, entry, submit, variant):
        """-> (rc, the batch whose ticket a successful submit filled)"""
        jb, L = self.jb, self.L
        n = {"negative_n": -1, "null_path": 1, "bad_chain": 1}.get(variant, 0)
        b = self.batch(max(n, 0))
        if variant == "null_path":
            b["paths"][0] = None
        k = {"k0": 0, "k17": 17}.get(variant, 2)
        views = (jb.View * 34)(*[jb.View(0, 0, 8, 8, 0, 0)] * 34)
        groups = (jb.ViewGroup * 5)(*[jb.ViewGroup(jb.Resize(8, 8, 0, 0), 1, 0)] * 5)
        groups[0].n_views = 0 if variant == "n_views0" else 1
        groups[1].reserved = 1 if variant == "reserved1" else 0
        n_groups = {"n_groups0": 0, "n_groups5": 5}.get(variant, 2)
        colors = (jb.ColorChain * 34)()
        if variant == "bad_chain":
            colors[1].n_ops = 1
            colors[1].ops[0].op = 99
        extra = {"": [], "_crops": [None if variant == "null_rois" else (jb.Roi * 1)(jb.Roi(0, 0, 8, 8))],
                 "_views": [views, k], "_views_color": [views, k, colors], "_view_groups": [views, groups, n_groups],
                 "_view_groups_color": [views, groups, n_groups, colors]}[entry]
        if variant == "null_views":
            extra[0] = None
        if variant == "null_groups":
            extra[1] = None
        if variant == "null_colors":
            extra[-1] = None
        fn = getattr(L, "jb_batch_decoder_%s%s" % ("submit" if submit else "run", entry))
        last = None if variant == "null_ticket" else (ctypes.byref(b["id"]) if submit else (ctypes.c_double * 4)())
        rc = fn(None if variant == "null_decoder" else h, None if variant == "null_paths" else b["paths"], n, *extra,
                None if variant == "null_rgb" else b["rgb"], b["w"], b["h"], None if variant == "null_statuses" else b["st"], last)
        return rc, b

    def calls(self):
        h = self.create()
        for state in CALL_STATES:
            self.establish(h, STATE_REQUESTS[state])
            for submit in (False, True):
                for entry in ENTRIES:
                    for variant in self.variants(entry, submit):
                        flying = [self.fly(h) for _ in range({"busy": 1, "busy2": 2}.get(state, 0))]
                        rc, b = self.call(h, entry, submit, variant)
                        self.row("call:%s:%s%s:%s" % (state, "submit" if submit else "run", entry, variant), rc)
                        for f in flying:   # (oldest first)
                            self.land(h, f)
                        if submit and rc == 0:
                            self.land(h, b)
        self.L.jb_batch_decoder_destroy(h)

    # ---- arena and device regions, tickets ---------------------------------------------------------------------------
    def outputs(self):
        import torch
        L = self.L
        region = torch.empty(2 * 65536 + 256, dtype=torch.uint8, device="cuda:0")
        base = (region.data_ptr() + 255) & ~255
        vp, sz = ctypes.c_void_p, ctypes.c_size_t

        def many(h, ptrs, sizes, n):
            return L.jb_batch_decoder_set_device_outputs(h, (vp * 2)(*ptrs) if ptrs is not None else None,
                                                         (sz * 2)(*sizes) if sizes is not None else None, n)

        self.row("out:null:set_arena", L.jb_batch_decoder_set_arena(None, 4096))
        self.row("out:null:set_device_output", L.jb_batch_decoder_set_device_output(None, vp(base), 65536))
        self.row("out:null:set_device_outputs", many(None, [base, base + 65536], [65536, 65536], 2))
        for kind in ("single", "multi"):
            h = self.create(kind == "multi")
            row = lambda name, rc: self.row("out:%s:%s" % (kind, name), rc)
            row("set_arena(65536)", L.jb_batch_decoder_set_arena(h, 65536))
            row("set_arena(0)", L.jb_batch_decoder_set_arena(h, 0))
            row("set_device_output(pointer, 0)", L.jb_batch_decoder_set_device_output(h, vp(base), 0))
            row("set_device_output(NULL, 4096)", L.jb_batch_decoder_set_device_output(h, None, 4096))
            row("set_device_output(misaligned)", L.jb_batch_decoder_set_device_output(h, vp(base + 1), 4096))
            row("set_device_output(region)", L.jb_batch_decoder_set_device_output(h, vp(base), 65536))
            row("set_device_output(NULL, 0)", L.jb_batch_decoder_set_device_output(h, None, 0))
            row("set_device_outputs(n=1)", many(h, [base, 0], [65536, 0], 1))
            row("set_device_outputs(n=1, off)", many(h, [None, None], [0, 0], 1))
            row("set_device_outputs(n=2)", many(h, [base, base + 65536], [65536, 65536], 2))
            row("set_device_outputs(n=3)", many(h, [base, base + 65536], [65536, 65536], 3))
            row("set_device_outputs(n=2, NULL arrays)", many(h, None, None, 2))
            row("set_device_outputs(n=2, a NULL pointer)", many(h, [base, None], [65536, 65536], 2))
            row("set_device_outputs(n=2, a size 0)", many(h, [base, base + 65536], [65536, 0], 2))
            row("set_device_outputs(n=2, misaligned)", many(h, [base, base + 65536 + 1], [65536, 4096], 2))
            row("set_device_outputs(n=0)", many(h, None, None, 0))
            b = self.fly(h)
            row("busy:set_arena(65536)", L.jb_batch_decoder_set_arena(h, 65536))
            row("busy:set_device_output(region)", L.jb_batch_decoder_set_device_output(h, vp(base), 65536))
            row("busy:set_device_outputs(n=1)", many(h, [base, 0], [65536, 0], 1))
            row("busy:set_device_outputs(n=2)", many(h, [base, base + 65536], [65536, 65536], 2))
            self.land(h, b)
            L.jb_batch_decoder_destroy(h)
        torch.cuda.synchronize()

    def tickets(self):
        L = self.L
        h = self.create()
        self.row("collect:null_decoder", L.jb_batch_decoder_collect(None, 0, None))
        self.row("collect:nothing_in_flight", L.jb_batch_decoder_collect(h, 0, None))
        self.row("collect:negative", L.jb_batch_decoder_collect(h, -1, None))
        b = self.fly(h)
        self.row("collect:unknown", L.jb_batch_decoder_collect(h, b["id"].value + 5, None))
        self.row("collect:other_side", L.jb_batch_decoder_collect(h, b["id"].value + 1, None))
        self.row("collect:first", L.jb_batch_decoder_collect(h, b["id"], None))
        self.row("collect:again", L.jb_batch_decoder_collect(h, b["id"], None))
        self.land(h, b)
        L.jb_batch_decoder_destroy(h)


def cases(jb, paths):
    """-> [(case name, return code, text), ...] of the loaded library; paths: tiny_files()"""
    d = _Driver(jb, paths)
    d.setters()
    d.calls()
    d.outputs()
    d.tickets()
    names = [r[0] for r in d.rows]
    assert len(set(names)) == len(names)
    return d.rows


def pure_names():
    """the names of the rows that tools/fuzz/batch_request_check prints: setters with nothing in flight whose argument passes the
    setter's own check, and entry points on a decoder with nothing in flight whose fixed arguments (decoder, paths, outputs,
    count) are good"""
    names = []
    for q in requests():
        for name, args in SETTERS:
            names += ["set:%s:idle:%s(%s)" % (request_name(q), name, arg) for arg, own in args if not own]
    d = _Driver.__new__(_Driver)
    fixed = ("null_decoder", "null_paths", "null_rgb", "null_statuses", "negative_n", "null_ticket", "null_path")
    for state in CALL_STATES[:5]:
        for submit in (False, True):
            for entry in ENTRIES:
                names += ["call:%s:%s%s:%s" % (state, "submit" if submit else "run", entry, v) for v in d.variants(entry, submit) if v not in fixed]
    return names
