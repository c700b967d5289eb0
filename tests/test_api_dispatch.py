"""The Python binding's dispatch, host side (no GPU, no library): which C entry point a call reaches, with which
arguments, and what comes back.  api._lib is replaced by a stub that records every jb_* call; Context and BatchDecoder are
bare objects.  The expectations are written from the rule, not computed by the binding:

  a rectangle or a target size with a scale other than 1 is JbError(-9), in that order; then a target size gives the
  _resized entry point, else a rectangle _roi, else a format (format 0 too) at scale 1 _fmt, else scale 1 the plain one,
  else _scaled -- where a planar format is JbError(-9) and format 0 is ignored, the output being [H, W, 3] uint8."""
import ctypes
import itertools
import os

import numpy as np
import pytest

PX = np.arange(64, dtype=np.uint8) * 3 + 1     # the "pixels" every stubbed decode returns: 2 x 2, any format
DT = {0: np.uint8, 1: np.uint8, 2: np.float32, 3: np.float16}
REFUSALS = {"roi": "a rectangle (roi) cannot be combined with a scale",
            "resize": "a target size (resize) cannot be combined with a scale",
            "fmt": "an output format cannot be combined with a scale"}


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


class StubLib:
    """Every jb_* attribute records (name, args) and returns 0 (rc of the batch calls: self.rc).  The decode entry points
    fill their three out-parameters; the batch entry points fill their arrays with `images` pointers (0 = failed)."""

    def __init__(self, images=()):
        self.calls, self.rc = [], 0
        self.images = list(images)          # addresses the batch entry points hand out
        self.flights, self.next_id = {}, 7

    def freed(self):
        return [a[0].value if isinstance(a[0], ctypes.c_void_p) else a[0] for n, a in self.calls if n == "jb_free"]

    def _fill(self, rgb, w, h, st, times):
        for i, p in enumerate(self.images):
            rgb[i], w[i], h[i], st[i] = p or None, 2, 2, 0 if p else -8
        if times is not None:
            times[0], times[1], times[2], times[3] = 1.0, 2.0, 3.0, 4.0

    def __getattr__(self, name):
        if not name.startswith("jb_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name == "jb_last_error":
                return b"stub error text"
            if name.startswith(("jb_decode_file", "jb_decode_memory")):
                args[-3]._obj.value, args[-2]._obj.value, args[-1]._obj.value = PX.ctypes.data, 2, 2
            elif name == "jb_batch_decoder_create":
                args[-1]._obj.value = 0x4321
            elif name == "jb_decode_batch":
                self._fill(*args[4:9])
                return self.rc
            elif name == "jb_batch_decoder_run":
                self._fill(*args[3:8])
                return self.rc
            elif name == "jb_batch_decoder_submit":
                args[-1]._obj.value = self.next_id
                self.flights[self.next_id] = args[3:7]
                self.next_id += 1
            elif name == "jb_batch_decoder_collect":
                arrays = self.flights.pop(args[1].value, None)
                if arrays is None:
                    return -7
                self._fill(*arrays, args[2])
                return self.rc
            return 0
        return call


@pytest.fixture
def stub(jb, monkeypatch):
    from jpeg_decoder_amd import api
    s = StubLib()
    monkeypatch.setattr(api, "_lib", s)
    return s


def _bare_ctx(jb):
    ctx = object.__new__(jb.Context)
    ctx._h = ctypes.c_void_p()     # (NULL: nothing for __del__ to destroy)
    return ctx


def _expected(jb, scale, fmt, roi, resize):
    """The rule of the module's docstring -> ("refused", text) or (route, the format number the output is shaped by)."""
    if roi is not None and scale != 1:
        return "refused", REFUSALS["roi"]
    if resize is not None and scale != 1:
        return "refused", REFUSALS["resize"]
    number = fmt.format if isinstance(fmt, jb.OutputSpec) else fmt
    if resize is not None:
        return "resized", number or 0
    if roi is not None:
        return "roi", number or 0
    if scale == 1:
        return ("plain", 0) if number is None else ("fmt", number)
    if number not in (None, 0):
        return "refused", REFUSALS["fmt"]
    return "scaled", 0


def _check_tail(jb, route, tail, scale, fmt, roi, resize):
    """The arguments between the family's own and its outputs: NULL against pointer for the rectangle and the spec, and
    what the pointers point at."""
    def spec_ok(arg):
        if fmt is None:
            return arg is None
        s = arg._obj
        return isinstance(s, jb.OutputSpec) and s.format == (fmt.format if isinstance(fmt, jb.OutputSpec) else fmt) and \
            (s is fmt or not isinstance(fmt, jb.OutputSpec))

    def roi_ok(arg):
        if roi is None:
            return arg is None
        r = arg._obj
        return isinstance(r, jb.Roi) and (r.x, r.y, r.width, r.height) == (3, 5, 20, 10) and (r is roi or not isinstance(roi, jb.Roi))

    if route == "resized":
        assert len(tail) == 4 and roi_ok(tail[0]) and tail[1:3] == (31, 17) and spec_ok(tail[3]), tail
    elif route == "roi":
        assert len(tail) == 2 and tail[0] is not None and roi_ok(tail[0]) and spec_ok(tail[1]), tail
    elif route == "fmt":
        assert len(tail) == 1 and tail[0] is not None and spec_ok(tail[0]), tail
    elif route == "scaled":
        assert tail == (scale,), tail
    else:
        assert tail == (), tail


def _cross(jb):
    fmts = (None, 0, 1, jb.OutputSpec.make(0), jb.OutputSpec.make(2))
    rois = (None, (3, 5, 20, 10), jb.Roi(3, 5, 20, 10))
    return list(itertools.product((1, 2), fmts, rois, (None, (31, 17))))


SYMBOL = {"plain": "", "scaled": "_scaled", "fmt": "_fmt", "roi": "_roi", "resized": "_resized"}


@pytest.mark.parametrize("family", ["jb_decode_file", "jb_decode_memory", "jb_blocks_to_rgb_device"])
def test_every_request_reaches_its_entry_point(jb, stub, family):
    ctx = _bare_ctx(jb)
    data = b"\xff\xd8 not a jpeg"
    batch = jb.DeviceBatch()
    stream = ctypes.c_void_p(0x77)
    cases = _cross(jb)
    assert len(cases) == 60
    seen = set()
    for scale, fmt, roi, resize in cases:
        kw = dict(scale=scale, fmt=fmt, roi=roi, resize=resize)
        if family == "jb_decode_file":
            def call():
                return ctx.decode_file("some/file.jpg", **kw)
        elif family == "jb_decode_memory":
            def call():
                return ctx.decode_memory(data, **kw)
        else:
            def call():
                return ctx.blocks_to_rgb_device(batch, stream, **kw)
        del stub.calls[:]
        route, what = _expected(jb, scale, fmt, roi, resize)
        seen.add(route)
        if route == "refused":
            with pytest.raises(jb.JbError) as e:
                call()
            assert e.value.status == -9 and str(e.value) == "JB_ERR_UNSUPPORTED: " + what, (kw, str(e.value))
            assert stub.calls == [], "refused before any call into the library"
            continue
        got = call()
        assert [n for n, _ in stub.calls if n != "jb_free"] == [family + SYMBOL[route]], (kw, stub.calls)
        args = stub.calls[0][1]
        assert args[0] is ctx._h
        if family == "jb_blocks_to_rgb_device":
            assert args[1]._obj is batch and args[-1] is stream
            _check_tail(jb, route, args[2:-1], scale, fmt, roi, resize)
            assert got is None and stub.freed() == []
            continue
        if family == "jb_decode_file":
            assert args[1] == os.fsencode("some/file.jpg")
            tail = args[2:-3]
        else:
            assert bytes((ctypes.c_char * args[2]).from_address(args[1].value)) == data
            tail = args[3:-3]
        _check_tail(jb, route, tail, scale, fmt, roi, resize)
        assert stub.freed() == [PX.ctypes.data], "exactly one jb_free, of the returned pointer"
        dt = np.dtype(DT[what])
        want = PX[:12 * dt.itemsize].view(dt).reshape((2, 2, 3) if what == 0 else (3, 2, 2))
        assert got.dtype == dt and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8)), kw
        assert not np.shares_memory(got, PX), "a copy: the buffer has been released"
    assert seen == {"refused", "plain", "scaled", "fmt", "roi", "resized"}


def test_a_failing_decode_raises_with_the_library_text_and_frees_nothing(jb, stub, monkeypatch):
    ctx = _bare_ctx(jb)
    monkeypatch.setattr(stub, "jb_decode_memory_roi", lambda *a: -2, raising=False)
    with pytest.raises(jb.JbError) as e:
        ctx.decode_memory(b"xx", roi=(3, 5, 20, 10))
    assert e.value.status == -2 and "stub error text" in str(e.value)
    assert stub.freed() == []
    assert [a for n, a in stub.calls if n == "jb_last_error"][0][0] is ctx._h


# ---- the batch path ----------------------------------------------------------------------------------
def _bare_decoder(jb, fmt=None, arena=False, device_out=False):
    dec = object.__new__(jb.BatchDecoder)
    dec._h = ctypes.c_void_p()
    dec._arena, dec._device_out, dec._flights, dec._fmt, dec._device = arena, device_out, {}, fmt, 0
    return dec


def _buffers():
    """Three decoded images (48 bytes each: 2 x 2 in any format) with a failed one in between."""
    bufs = [np.arange(48, dtype=np.uint8) + 10 * k for k in range(3)]
    return bufs, [bufs[0].ctypes.data, 0, bufs[1].ctypes.data, bufs[2].ctypes.data]


PATHS = ["a.jpg", "b.jpg", "c.jpg", "d.jpg"]
TIMES = {"wall_s": 1.0, "entropy_s": 2.0, "device_s": 3.0, "read_s": 4.0}


def _check_host_results(stub, result, bufs, ptrs, fmt=0, keep_pixels=True, freed=True, rc=0):
    imgs, st, t = result
    dt = np.dtype(DT[fmt])
    live = [bufs[0], None, bufs[1], bufs[2]]
    assert len(imgs) == 4 and imgs[1] is None
    for i, b in enumerate(live):
        if b is None:
            continue
        if not keep_pixels:
            assert imgs[i] == (2, 2)
            continue
        want = b[:12 * dt.itemsize].view(dt).reshape((2, 2, 3) if fmt == 0 else (3, 2, 2))
        assert imgs[i].dtype == dt and imgs[i].shape == want.shape and np.array_equal(imgs[i], want), i
        assert not np.shares_memory(imgs[i], b)
    assert st == [0, -8, 0, 0]
    assert t == dict(TIMES, rc=rc, error="stub error text" if rc else "")
    assert sorted(stub.freed()) == (sorted(p for p in ptrs if p) if freed else [])


def test_decode_batch_and_its_callback(jb, stub):
    bufs, ptrs = _buffers()
    stub.images = ptrs
    result = jb.decode_batch(PATHS, n_threads=3, device=1)
    name, args = stub.calls[0]
    assert name == "jb_decode_batch" and args[0] == 1 and list(args[1]) == [os.fsencode(p) for p in PATHS] and args[2:4] == (4, 3)
    assert [n for n, _ in stub.calls if n not in ("jb_free", "jb_last_error")] == ["jb_decode_batch"]
    _check_host_results(stub, result, bufs, ptrs)
    # the callback sees a view of every decoded image before its buffer is released; no pixels are kept
    del stub.calls[:]
    seen = []
    result = jb.decode_batch(PATHS, keep_pixels=False, on_image=lambda i, v: seen.append((i, v.copy(), len(stub.freed()))))
    _check_host_results(stub, result, bufs, ptrs, keep_pixels=False)
    assert [(i, n) for i, _, n in seen] == [(0, 0), (2, 1), (3, 2)]
    for (i, v, _), b in zip(seen, bufs):
        assert v.shape == (2, 2, 3) and np.array_equal(v.ravel(), b[:12])
    # a failing status is reported with the library's text, and what was decoded is still delivered
    del stub.calls[:]
    stub.rc = -8
    _check_host_results(stub, jb.decode_batch(PATHS), bufs, ptrs, rc=-8)


def test_decode_batch_with_a_scale_goes_through_a_temporary_decoder(jb, stub):
    bufs, ptrs = _buffers()
    stub.images = ptrs
    result = jb.decode_batch(PATHS, n_threads=8, device=0, scale=4)
    names = [n for n, _ in stub.calls if n not in ("jb_free", "jb_last_error")]
    assert names == ["jb_batch_decoder_create", "jb_batch_decoder_set_scale", "jb_batch_decoder_run", "jb_batch_decoder_destroy"]
    assert stub.calls[0][1][:2] == (0, 4), "no more threads than files"
    assert stub.calls[1][1][1] == 4
    _check_host_results(stub, result, bufs, ptrs)


@pytest.mark.parametrize("fmt", [None, 0, 2, 3])
@pytest.mark.parametrize("arena", [False, True])
def test_batch_decoder_run(jb, stub, fmt, arena):
    bufs, ptrs = _buffers()
    stub.images = ptrs
    dec = _bare_decoder(jb, None if fmt is None else jb.OutputSpec.make(fmt), arena=arena)
    result = dec.run(PATHS)
    name, args = stub.calls[0]
    assert name == "jb_batch_decoder_run" and args[0] is dec._h and list(args[1]) == [os.fsencode(p) for p in PATHS] and args[2] == 4
    _check_host_results(stub, result, bufs, ptrs, fmt or 0, freed=not arena)   # arena images belong to the decoder


def test_batch_decoder_run_to_device(jb, stub):
    bufs, ptrs = _buffers()
    stub.images = ptrs
    dec = _bare_decoder(jb, arena=True, device_out=True)
    with pytest.raises(AssertionError):
        dec.run(PATHS)
    got, dims, st, t = dec.run_to_device(PATHS)
    assert got == ptrs and all(type(p) is int for p in got) and dims == [(2, 2)] * 4 and st == [0, -8, 0, 0]
    assert t == dict(TIMES, rc=0, error="") and stub.freed() == []
    assert [n for n, _ in stub.calls] == ["jb_batch_decoder_run"]
    with pytest.raises(AssertionError):
        _bare_decoder(jb).run_to_device(PATHS)


def test_batch_decoder_submit_and_collect(jb, stub):
    bufs, ptrs = _buffers()
    stub.images = ptrs
    dec = _bare_decoder(jb, jb.OutputSpec.make(3))
    t0, t1 = dec.submit(PATHS), dec.submit(PATHS[::-1])
    for t, ident in ((t0, 7), (t1, 8)):
        assert {"id", "n", "rgb", "w", "h", "st"} <= set(t) and t["n"] == 4 and t["id"].value == ident
        assert dec._flights[ident] is t, "the decoder keeps the arrays of a batch in flight alive"
    name, args = stub.calls[0]
    assert name == "jb_batch_decoder_submit" and args[0] is dec._h and list(args[1]) == [os.fsencode(p) for p in PATHS] and args[2] == 4
    assert (args[3], args[4], args[5], args[6]) == (t0["rgb"], t0["w"], t0["h"], t0["st"])
    del stub.calls[:]
    _check_host_results(stub, dec.collect(t0), bufs, ptrs, 3)
    assert stub.calls[0][0] == "jb_batch_decoder_collect" and stub.calls[0][1][:2] == (dec._h, t0["id"])
    assert list(dec._flights) == [8]
    # device output: what run_to_device returns
    dec._arena = dec._device_out = True
    del stub.calls[:]
    got, dims, st, t = dec.collect(t1)
    assert got == ptrs and dims == [(2, 2)] * 4 and st == [0, -8, 0, 0] and t == dict(TIMES, rc=0, error="")
    assert stub.freed() == [] and dec._flights == {}


def test_a_second_collect_of_one_ticket_frees_nothing(jb, stub):
    """NEW BEHAVIOUR (the binding before this test existed fails both assertions marked so): the library answers a
    second collect of one ticket with JB_ERR_STATE, and the ticket's pointers were released by the first."""
    bufs, ptrs = _buffers()
    stub.images = ptrs
    dec = _bare_decoder(jb)
    t0 = dec.submit(PATHS)
    _check_host_results(stub, dec.collect(t0), bufs, ptrs)
    del stub.calls[:]
    seen = []
    imgs, st, t = dec.collect(t0, on_image=lambda i, v: seen.append(i))
    assert t["rc"] == -7 and t["error"] == "stub error text"
    assert stub.freed() == [], "NEW: the second collect() of one ticket calls jb_free zero times"
    assert [im is None for im in imgs] == [True] * 4 and seen == [], "NEW: collect() after a -7 reads no pointer"
    assert len(st) == 4


def test_collect_of_an_unknown_ticket_touches_no_pointer(jb, stub):
    """NEW BEHAVIOUR, as above: a ticket the decoder does not know (another decoder's, say) keeps its arrays as they are;
    with device output every pointer comes back 0."""
    bufs, ptrs = _buffers()
    stub.images = ptrs
    other = _bare_decoder(jb)
    ticket = other.submit(PATHS)
    stub.flights.clear()                       # (the library has no such batch)
    for i, p in enumerate(ptrs):               # pointers somebody else owns: live memory here, so a read is seen, not fatal
        ticket["rgb"][i] = p or None
    dec = _bare_decoder(jb)
    del stub.calls[:]
    seen = []
    imgs, st, t = dec.collect(ticket, on_image=lambda i, v: seen.append(i))
    assert t["rc"] == -7
    assert [im is None for im in imgs] == [True] * 4 and seen == [] and stub.freed() == [], "NEW: collect() after a -7 reads no pointer"
    assert [int(p or 0) for p in ticket["rgb"]] == ptrs, "and the ticket is left as it was"
    dec._arena = dec._device_out = True
    got, dims, st, t = dec.collect(ticket)
    assert t["rc"] == -7 and got == [0] * 4 and len(dims) == 4 and len(st) == 4, "NEW: device output: every pointer 0"
