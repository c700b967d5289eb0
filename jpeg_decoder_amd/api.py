"""ctypes binding of include/jpegblk.h (libjpegblk.so).  One Python function per C entry point;
no arithmetic happens on this side."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# JPEGBLK_LIB: experiment builds of the same ABI (tools/); the product is libjpegblk.so
_LIB_PATH = os.environ.get("JPEGBLK_LIB") or os.path.join(_HERE, "libjpegblk.so")

JB_OK = 0
STATUS_NAMES = {0: "JB_OK", -1: "JB_ERR_NULL", -2: "JB_ERR_GEOMETRY", -3: "JB_ERR_SAMPLING",
                -4: "JB_ERR_QTAB", -5: "JB_ERR_CAPACITY", -6: "JB_ERR_HIP", -7: "JB_ERR_STATE",
                -8: "JB_ERR_FORMAT", -9: "JB_ERR_UNSUPPORTED"}


class JbError(RuntimeError):
    def __init__(self, status, text=""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {text}")


class ImageDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hs", ctypes.c_int32), ("vs", ctypes.c_int32),
                ("qtab_id", ctypes.c_int32 * 3), ("reserved", ctypes.c_int32)]


class Geometry(ctypes.Structure):
    _fields_ = [("mcu_w", ctypes.c_int32), ("mcu_h", ctypes.c_int32),
                ("mcu_w_real", ctypes.c_int32), ("mcu_h_real", ctypes.c_int32),
                ("mcus_x", ctypes.c_int32), ("mcus_y", ctypes.c_int32),
                ("blocks_per_mcu", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("n_coded_blocks", ctypes.c_int64), ("coef_bytes", ctypes.c_int64),
                ("rgb_bytes", ctypes.c_int64)]


class DeviceBatch(ctypes.Structure):
    _fields_ = [("desc", ImageDesc), ("n_images", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("d_coef", ctypes.c_void_p), ("coef_image_stride", ctypes.c_int64),
                ("d_qtabs", ctypes.c_void_p), ("qtab_image_stride", ctypes.c_int64),
                ("d_rgb", ctypes.c_void_p), ("rgb_image_stride", ctypes.c_int64),
                ("rgb_row_stride", ctypes.c_int64)]


# output formats (jpegblk.h, "tensor-ready output"): 0 = interleaved uint8 [H, W, 3], the others planar [3, H, W]
FMT_RGB_U8_HWC, FMT_RGB_U8_CHW, FMT_RGB_F32_CHW, FMT_RGB_F16_CHW = 0, 1, 2, 3
FMT_DTYPE = {FMT_RGB_U8_HWC: np.uint8, FMT_RGB_U8_CHW: np.uint8, FMT_RGB_F32_CHW: np.float32, FMT_RGB_F16_CHW: np.float16}
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class OutputSpec(ctypes.Structure):
    """jb_output_spec.  OutputSpec.make(format, scale=(1, 1, 1), bias=(0, 0, 0)): value = f32(u8) * scale[c] + bias[c]
    (float formats; scale / bias are rounded to float32 here, as the C struct holds them)."""
    _fields_ = [("format", ctypes.c_int32), ("reserved", ctypes.c_int32), ("plane_stride", ctypes.c_int64),
                ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3)]

    @classmethod
    def make(cls, format, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0), plane_stride=0):
        s = cls()
        s.format, s.reserved, s.plane_stride = int(format), 0, int(plane_stride)
        for c in range(3):
            s.scale[c], s.bias[c] = float(scale[c]), float(bias[c])
        return s

    @classmethod
    def imagenet(cls, format=FMT_RGB_F32_CHW):
        """(x / 255 - mean) / std as one multiply and one add: scale = 1 / (255 * std), bias = -mean / std."""
        return cls.make(format, [1.0 / (255.0 * sd) for sd in IMAGENET_STD], [-m / sd for m, sd in zip(IMAGENET_MEAN, IMAGENET_STD)])

    @property
    def dtype(self):
        return FMT_DTYPE[self.format]


class Roi(ctypes.Structure):
    """jb_roi: a rectangle (x, y, width, height) in pixels of the full-size image."""
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


# resampling filters (jpegblk.h, "resampling filters"): 0 = the exact area resize, the others Pillow's 8-bit resampling
FILTER_AREA, FILTER_BILINEAR, FILTER_BICUBIC = 0, 1, 2
# "decoder arithmetic" (include/jpegblk.h): the reference program's, or libjpeg's -- Pillow's decode bit for bit
ARITH_REFERENCE, ARITH_LIBJPEG = 0, 1
# "orientation" (include/jpegblk.h): the file's Exif tag, or the pixels as stored; 2..8 are the Exif codes themselves
ORIENT_EXIF, ORIENT_STORED = 0, 1


class Resize(ctypes.Structure):
    """jb_resize: a target size and the filter that gets there."""
    _fields_ = [("out_w", ctypes.c_int32), ("out_h", ctypes.c_int32), ("filter", ctypes.c_int32), ("reserved", ctypes.c_int32)]


VIEW_MIRROR = 1   # jb_view.flags bit 0 (jpegblk.h, "views"): mirror the OUTPUT left-right
VIEWS_MAX = 16


class View(ctypes.Structure):
    """jb_view: a rectangle as jb_roi, and flags (VIEW_MIRROR)."""
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32)]


VIEW_GROUPS_MAX = 4


class ViewGroup(ctypes.Structure):
    """jb_view_group ("view groups"): n_views views per image under one target size and filter."""
    _fields_ = [("rs", Resize), ("n_views", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class ViewOutput(ctypes.Structure):
    """jb_view_output: where a group's outputs go -- output (i, v) at d_out + i * image_stride + v * view_stride, rows
    row_stride apart, the planes of a planar format plane_stride apart (0: tight)."""
    _fields_ = [("d_out", ctypes.c_void_p), ("image_stride", ctypes.c_int64), ("view_stride", ctypes.c_int64),
                ("row_stride", ctypes.c_int64), ("plane_stride", ctypes.c_int64)]


# jb_color_op.op (jpegblk.h, "colour chains")
COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION, COLOR_HUE, COLOR_GRAYSCALE, COLOR_SOLARIZE = 1, 2, 3, 4, 5, 6
COLOR_BLUR = 16               # (neighbourhood operations are numbered from 16); value: Pillow's GaussianBlur radius
COLOR_POSTERIZE, COLOR_INVERT, COLOR_AUTOCONTRAST, COLOR_EQUALIZE = 10, 11, 12, 13   # RandAugment's pointwise and table operations
COLOR_SHARPNESS = 17          # a neighbourhood operation; value: ImageEnhance.Sharpness' factor
# geometric operations (numbered from 32): torchvision's affine entries at NEAREST with a black fill, Pillow's bits; value: the
# shear (a tangent), the translation in pixels (integral), the rotation in degrees
COLOR_SHEAR_X, COLOR_SHEAR_Y, COLOR_TRANSLATE_X, COLOR_TRANSLATE_Y, COLOR_ROTATE = 32, 33, 34, 35, 36
COLOR_WARPS_MAX = 2           # geometric operations a chain may hold, none of them behind a COLOR_BLUR / COLOR_SHARPNESS
WARP_SHIFT, WARP_FIXED = 0, 1  # warp_params' modes: Pillow's integer shift, its 16.16 fixed-point path
COLOR_OPS_MAX = 8
COLOR_STATS_MAX = 2           # statistics operations (contrast, autocontrast, equalize) a chain may hold, one of them a contrast
COLOR_BLUR_BOX_MAX = 7        # the largest box radius of a COLOR_BLUR (Gaussian radii up to about 8.4)


class ColorOp(ctypes.Structure):
    """jb_color_op: one operation of a colour chain, (COLOR_*, a float32 value)."""
    _fields_ = [("op", ctypes.c_int32), ("value", ctypes.c_float)]


class ColorChain(ctypes.Structure):
    """jb_color_chain ("colour chains"): 0..8 operations applied in order to the uint8 pixels of one view."""
    _fields_ = [("n_ops", ctypes.c_int32), ("reserved", ctypes.c_int32), ("ops", ColorOp * COLOR_OPS_MAX)]

    @classmethod
    def make(cls, chain):
        """None / [] (the identity) / [(op, value), ...] / a ColorChain -> a ColorChain.  More than 8 operations: n_ops says
        so and holds the first 8 -- jb_color_check refuses it, as it refuses every other bad chain."""
        if isinstance(chain, cls):
            return chain
        ops = [o if isinstance(o, ColorOp) else ColorOp(int(o[0]), float(o[1])) for o in (chain or [])]
        c = cls()
        c.n_ops = len(ops)
        for i, o in enumerate(ops[:COLOR_OPS_MAX]):
            c.ops[i] = o
        return c


def _chain_array(chains):
    """a flat list of chains -> a ctypes array of jb_color_chain, at least one element long.  Chains of plain (op, value)
    pairs -- what color.py draws -- are packed through numpy in bulk (a batch has thousands); anything else one by one."""
    import numpy as np
    chains = [c if c is not None else () for c in chains]
    n = len(chains)
    if any(isinstance(c, ColorChain) or any(isinstance(o, ColorOp) for o in c) for c in chains):
        flat = [ColorChain.make(c) for c in chains]
        return (ColorChain * max(n, 1))(*flat)
    rec = np.zeros(max(n, 1), dtype=[("n_ops", "<i4"), ("reserved", "<i4"), ("op", "<i4", (COLOR_OPS_MAX,)), ("value", "<f4", (COLOR_OPS_MAX,))])
    lens = np.array([len(c) for c in chains], dtype=np.int64).reshape(-1)
    rec["n_ops"][:n] = lens                     # (more than 8: n_ops says so, jb_color_check refuses)
    pairs = [(int(o[0]), float(o[1])) for c in chains for o in c[:COLOR_OPS_MAX]]
    if pairs:
        kept = np.minimum(lens, COLOR_OPS_MAX)
        rows = np.repeat(np.arange(n), kept)
        cols = np.arange(len(pairs)) - np.repeat(np.cumsum(kept) - kept, kept)
        flat = np.array(pairs, dtype=np.float64)
        rec["op"][rows, cols] = flat[:, 0].astype(np.int32)
        rec["value"][rows, cols] = flat[:, 1].astype(np.float32)
    # jb_color_op is (op, value) interleaved: weave the two columns into the ABI's layout
    out = np.zeros(max(n, 1), dtype=[("n_ops", "<i4"), ("reserved", "<i4"), ("ops", [("op", "<i4"), ("value", "<f4")], (COLOR_OPS_MAX,))])
    out["n_ops"], out["ops"]["op"], out["ops"]["value"] = rec["n_ops"], rec["op"], rec["value"]
    assert out.dtype.itemsize == ctypes.sizeof(ColorChain)
    return (ColorChain * max(n, 1)).from_buffer(out)   # (the array keeps `out` alive)


def _color_array(colors, n, k):
    """colors=[[chain, ... K], ... N] -> a ctypes array of N * K jb_color_chain parallel to the views; another shape than the
    views': JbError(-2)"""
    rows = [list(r) for r in colors]
    if len(rows) != n or any(len(r) != k for r in rows):
        raise JbError(-2, f"colors: {n} rows of {k} chains wanted, parallel to the views")
    return _chain_array([c for r in rows for c in r])


def _group_array(view_groups):
    """[(k, (w, h)[, filter]) or ViewGroup, ... G] -> (a ctypes array of G jb_view_group, at least one element long, G)."""
    gs = []
    for g in view_groups:
        if not isinstance(g, ViewGroup):
            g = tuple(g)
            g = ViewGroup(Resize(int(g[1][0]), int(g[1][1]), int(g[2]) if len(g) > 2 else FILTER_AREA, 0), int(g[0]), 0)
        gs.append(g)
    return (ViewGroup * max(len(gs), 1))(*gs), len(gs)


def _output_array(view_outputs, n_groups):
    """[(d_out, image_stride, view_stride, row_stride[, plane_stride]) or ViewOutput, ... G] -> a ctypes array of jb_view_output;
    another count than the groups': JbError(-2)."""
    outs = [o if isinstance(o, ViewOutput) else ViewOutput(*([int(v) for v in o] + [0] * (5 - len(o)))) for o in view_outputs]
    if len(outs) != n_groups:
        raise JbError(-2, f"{len(outs)} view outputs for {n_groups} groups")
    return (ViewOutput * max(len(outs), 1))(*outs)


# "fit" (include/jpegblk.h): what a target size does with a source of another aspect ratio -- stretch it (the default), scale
# it to fit inside and fill the rest (letterbox), or cut the largest centred rectangle of the target's aspect ratio
FIT_STRETCH, FIT_PAD, FIT_COVER = 0, 1, 2
FIT_CENTER, FIT_START, FIT_END = 0, 1, 2


class Fit(ctypes.Structure):
    """jb_fit: a mode (FIT_*), an anchor (FIT_CENTER / FIT_START / FIT_END) and, for FIT_PAD, the border's colour."""
    _fields_ = [("mode", ctypes.c_int32), ("anchor", ctypes.c_int32), ("fill", ctypes.c_uint8 * 3), ("reserved8", ctypes.c_uint8),
                ("reserved", ctypes.c_int32)]

    @classmethod
    def pad(cls, fill=(0, 0, 0), anchor=FIT_CENTER):
        """Letterbox: the source scaled to fit inside the target (Pillow's ImageOps.pad), the rest filled with `fill`."""
        r, g, b = [int(v) for v in fill]
        return cls(FIT_PAD, int(anchor), (ctypes.c_uint8 * 3)(r, g, b), 0, 0)

    @classmethod
    def cover(cls, anchor=FIT_CENTER):
        """The largest rectangle of the target's aspect ratio, centred (or anchored), resized to the target."""
        return cls(FIT_COVER, int(anchor), (ctypes.c_uint8 * 3)(0, 0, 0), 0, 0)


def _fit_struct(fit):
    """None / a mode number / a Fit -> a Fit, or None for what asks for nothing new (None, FIT_STRETCH with nothing else set)."""
    if fit is None:
        return None
    if not isinstance(fit, Fit):
        fit = Fit(int(fit), FIT_CENTER, (ctypes.c_uint8 * 3)(0, 0, 0), 0, 0)
    if fit.mode == FIT_STRETCH and fit.anchor == 0 and fit.reserved8 == 0 and fit.reserved == 0:
        return None
    return fit


class FitGeometry(ctypes.Structure):
    """jb_fit_geometry: what is resampled (src, in the frame) and where it lands (inner, in the target)."""
    _fields_ = [("src", Roi), ("inner", Roi)]


class DraftGeometry(ctypes.Structure):
    """jb_draft_geometry: the draft frame, the luma and chroma block sizes and what the upsampler still does."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("luma_block", ctypes.c_int32), ("chroma_block", ctypes.c_int32),
                ("up_h", ctypes.c_int32), ("up_v", ctypes.c_int32), ("fancy", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _ref(struct):
    """byref(struct), or None (a NULL pointer) for None."""
    return ctypes.byref(struct) if struct is not None else None


def _crop_array(crops, n=None):
    """[(x, y, w, h) or Roi, ...] -> a ctypes array of jb_roi (at least one element long, so that it is never NULL);
    n: the count the call wants (JbError(-2) for another)."""
    crops = list(crops)
    if n is not None and len(crops) != n:
        raise JbError(-2, f"{len(crops)} rectangles (crops) for {n} images")
    rois = [c if isinstance(c, Roi) else Roi(*[int(v) for v in c]) for c in crops]
    return (Roi * max(len(rois), 1))(*rois)


def _view_array(views, n=None):
    """[[(x, y, w, h[, mirror]) or View, ... K], ... N] -> (a ctypes array of N * K jb_view, image-major and at least one
    element long, K).  Rows of unequal length, or (n given) another count of rows than n: JbError(-2)."""
    rows = [list(r) for r in views]
    if n is not None and len(rows) != n:
        raise JbError(-2, f"{len(rows)} rows of views for {n} images")
    k = len(rows[0]) if rows else 1
    if any(len(r) != k for r in rows):
        raise JbError(-2, "views: every image wants the same number of views")
    flat = []
    for r in rows:
        for v in r:
            if isinstance(v, View):
                flat.append(v)
            else:
                v = tuple(v)
                flat.append(View(int(v[0]), int(v[1]), int(v[2]), int(v[3]), VIEW_MIRROR if len(v) > 4 and v[4] else 0, 0))
    return (View * max(len(flat), 1))(*flat), k


class _Request:
    """The output request of one call, normalised in this one place.  (scale, fmt, roi, resize, crops, filter) as the caller gave
    them (fmt: None / a format number / an OutputSpec; roi: None / (x, y, w, h) / a Roi; resize: None / (w, h); crops: None
    / a rectangle per image) become .scale, .spec (OutputSpec or None), .roi (Roi or None), .target ((w, h) or None) and
    .crops (a ctypes array of Roi or None; .n_crops).  A rectangle or a target size together with a scale other than 1 is
    JbError(-9), raised here: no C entry point takes the pair.  So are per-image rectangles with a scale or with roi (two
    rectangles for one image); without a target size they are JbError(-7): only a target makes the outputs one size.
    filter (FILTER_*) becomes .filter; FILTER_AREA asks for nothing new, any other filter without a target size is
    JbError(-7).  views (K views per image, [[(x, y, w, h[, mirror]), ...], ...]) become .views (a ctypes array of View or
    None; .n_view_rows images of .views_per_image each): with a scale, roi or crops JbError(-9), without a target size
    JbError(-7), rows of unequal length JbError(-2).  fit (None / a mode number / a Fit) becomes .fit (a Fit, or None for
    FIT_STRETCH, which asks for nothing new): a mode other than FIT_STRETCH without a target size is JbError(-7), with
    crops or views JbError(-9), behind every refusal above.  view_groups ([(k, (w, h)[, filter]), ...]: "view groups") become
    .groups (a ctypes array of ViewGroup; .n_groups) and bring their own targets and filters: with resize, a filter other
    than FILTER_AREA, roi, crops, a scale or a fit JbError(-9), without views JbError(-7), a row of views whose length is
    not the groups' K JbError(-2); view_outputs (the seam's jb_view_output per group) become .outputs.  colors ([[chain, ...
    K], ... N], a chain being None / [(op, value), ...]: "colour chains") become .colors (a ctypes array of ColorChain parallel
    to .views, or None): without views ValueError, another shape than the views' JbError(-2)."""

    def __init__(self, scale=1, fmt=None, roi=None, resize=None, crops=None, filter=FILTER_AREA, views=None, fit=None, view_groups=None,
                 view_outputs=None, colors=None):
        if colors is not None and views is None:
            raise ValueError("colors want views (a K = 1 views= call covers a plain one)")
        self.groups, self.n_groups, self.outputs = None, 0, None
        if view_groups is not None:
            if resize is not None or int(filter) != FILTER_AREA or roi is not None or crops is not None or scale != 1 or _fit_struct(fit) is not None:
                raise JbError(-9, "view groups bring their own targets and filters: not with resize, filter, roi, crops, a scale or a fit")
            if views is None:
                raise JbError(-7, "view groups want views")
            self.groups, self.n_groups = _group_array(view_groups)
            if view_outputs is not None:
                self.outputs = _output_array(view_outputs, self.n_groups)
        self.scale = scale
        self.filter = int(filter)
        if self.filter != FILTER_AREA and resize is None:
            raise JbError(-7, "a resampling filter wants a target size (resize)")
        self.spec = fmt if fmt is None or isinstance(fmt, OutputSpec) else OutputSpec.make(fmt)
        if roi is not None and scale != 1:
            raise JbError(-9, "a rectangle (roi) cannot be combined with a scale")
        if resize is not None and scale != 1:
            raise JbError(-9, "a target size (resize) cannot be combined with a scale")
        self.roi = roi if roi is None or isinstance(roi, Roi) else Roi(*[int(v) for v in roi])
        self.target = None
        if resize is not None:
            w, h = resize
            self.target = int(w), int(h)
        self.crops, self.n_crops = None, 0
        if crops is not None:
            if scale != 1:
                raise JbError(-9, "per-image rectangles (crops) cannot be combined with a scale")
            if roi is not None:
                raise JbError(-9, "per-image rectangles (crops) cannot be combined with a rectangle for every image (roi)")
            if resize is None:
                raise JbError(-7, "per-image rectangles (crops) want a target size (resize)")
            self.crops = _crop_array(crops)
            self.n_crops = len(list(crops))
        self.views, self.views_per_image, self.n_view_rows = None, 0, 0
        if views is not None:
            if scale != 1:
                raise JbError(-9, "views cannot be combined with a scale")
            if roi is not None:
                raise JbError(-9, "views cannot be combined with a rectangle for every image (roi)")
            if crops is not None:
                raise JbError(-9, "views cannot be combined with per-image rectangles (crops)")
            if resize is None and view_groups is None:
                raise JbError(-7, "views want a target size (resize)")
            views = [list(r) for r in views]
            if self.groups is not None and any(len(r) != sum(g.n_views for g in self.groups[:self.n_groups]) for r in views):
                raise JbError(-2, "view groups: every image wants as many views as the groups count")
            self.views, self.views_per_image = _view_array(views)
            self.n_view_rows = len(views)
        self.colors = None
        if colors is not None:
            self.colors = _color_array(colors, self.n_view_rows, self.views_per_image)
        self.fit = _fit_struct(fit)
        if self.fit is not None and self.fit.mode != FIT_STRETCH:
            if resize is None:
                raise JbError(-7, "a fit other than FIT_STRETCH wants a target size (resize)")
            if crops is not None or views is not None:
                raise JbError(-9, "a fit other than FIT_STRETCH cannot be combined with per-image rectangles (crops) or views")

    def routed(self):
        """-> (route, the arguments the route's entry points take between their family's own and their outputs).  The
        route names the variant of an entry point that takes this request (_ROUTES has the symbols).  A planar format
        with a scale has none, JbError(-9); format 0 with a scale is the scaled route, which takes no spec."""
        # (a mode other than FIT_STRETCH, which __init__ has refused together with crops or views and without a target size;
        # or a Fit that is none -- a bad mode, anchor or reserved field -- which C refuses whatever else the request holds:
        # crops and views are not passed on, no route takes them next to a fit)
        if self.fit is not None:
            rs = ctypes.byref(_resize_struct(self.target, self.filter))
            return "fit", (_ref(self.roi), rs, ctypes.byref(self.fit), _ref(self.spec))
        if self.groups is not None:      # (every group brings its jb_resize)
            if self.colors is not None:
                return "view_groups_color", (self.views, self.groups, self.outputs, self.n_groups, self.colors, _ref(self.spec))
            return "view_groups", (self.views, self.groups, self.outputs, self.n_groups, _ref(self.spec))
        if self.views is not None:       # (takes a jb_resize: the filter needs no route of its own)
            rs = ctypes.byref(Resize(self.target[0], self.target[1], self.filter, 0))
            if self.colors is not None:
                return "views_color", (self.views, self.views_per_image, rs, self.colors, _ref(self.spec))
            return "views", (self.views, self.views_per_image, rs, _ref(self.spec))
        if self.filter != FILTER_AREA:   # (always with a target size)
            rs = ctypes.byref(Resize(self.target[0], self.target[1], self.filter, 0))
            if self.crops is not None:
                return "crops_filtered", (self.crops, rs, _ref(self.spec))
            return "filtered", (_ref(self.roi), rs, _ref(self.spec))
        if self.crops is not None:
            return "crops", (self.crops, self.target[0], self.target[1], _ref(self.spec))
        if self.target is not None:
            return "resized", (_ref(self.roi), self.target[0], self.target[1], _ref(self.spec))
        if self.roi is not None:
            return "roi", (_ref(self.roi), _ref(self.spec))
        if self.scale == 1:
            return ("fmt", (_ref(self.spec),)) if self.spec is not None else ("plain", ())
        if self.spec is not None and self.spec.format != FMT_RGB_U8_HWC:
            raise JbError(-9, "an output format cannot be combined with a scale")
        return "scaled", (self.scale,)


# route -> its entry point in each family: decode(path), decode(bytes), the seam over device buffers.  The next output
# option is one more row here and one more return in _Request.routed().
_FILE, _MEMORY, _DEVICE = 0, 1, 2
_ROUTES = {"plain": ("jb_decode_file", "jb_decode_memory", "jb_blocks_to_rgb_device"),
           "scaled": ("jb_decode_file_scaled", "jb_decode_memory_scaled", "jb_blocks_to_rgb_device_scaled"),
           "fmt": ("jb_decode_file_fmt", "jb_decode_memory_fmt", "jb_blocks_to_rgb_device_fmt"),
           "roi": ("jb_decode_file_roi", "jb_decode_memory_roi", "jb_blocks_to_rgb_device_roi"),
           "resized": ("jb_decode_file_resized", "jb_decode_memory_resized", "jb_blocks_to_rgb_device_resized"),
           # (the device family alone: decode(path) and decode(bytes) handle one image, and have roi=)
           "crops": (None, None, "jb_blocks_to_rgb_device_crops"),
           # a filter other than FILTER_AREA (FILTER_AREA takes the two routes above)
           "filtered": ("jb_decode_file_filtered", "jb_decode_memory_filtered", "jb_blocks_to_rgb_device_filtered"),
           "crops_filtered": (None, None, "jb_blocks_to_rgb_device_crops_filtered"),
           # K views per image, each optionally mirrored, any filter
           "views": (None, None, "jb_blocks_to_rgb_device_views"),
           # the views of an image in up to four groups, each with its own target size and filter
           "view_groups": (None, None, "jb_blocks_to_rgb_device_view_groups"),
           # views / view groups with colors=: a colour chain per view, between the resize and the output format
           "views_color": (None, None, "jb_blocks_to_rgb_device_views_color"),
           "view_groups_color": (None, None, "jb_blocks_to_rgb_device_view_groups_color"),
           # a fit other than FIT_STRETCH: letterbox or centred crop to the target, any filter
           "fit": ("jb_decode_file_fit", "jb_decode_memory_fit", "jb_blocks_to_rgb_device_fit")}


def roi_check(desc, roi):
    """jb_roi_check: does the rectangle lie in the descriptor's image?  Raises JbError otherwise."""
    _check(lib().jb_roi_check(ctypes.byref(desc), ctypes.byref(_Request(roi=roi).roi)))


def resize_check(desc, resize, roi=None):
    """jb_resize_check: does the rectangle (None: the whole image) lie in the descriptor's image, and is the target
    size (w, h) in 1..65535?  Raises JbError otherwise."""
    q = _Request(roi=roi, resize=resize)
    w, h = q.target
    _check(lib().jb_resize_check(ctypes.byref(desc), _ref(q.roi), w, h))


def crops_check(desc, crops, resize):
    """jb_crops_check: does every rectangle of `crops` lie in the descriptor's image, and is the target size (w, h) in
    1..65535?  Raises JbError otherwise, the text naming the index of the first rectangle that does not."""
    q = _Request(resize=resize, crops=crops)
    bad = ctypes.c_int(-1)
    rc = lib().jb_crops_check(ctypes.byref(desc), q.crops, q.n_crops, q.target[0], q.target[1], ctypes.byref(bad))
    if rc != JB_OK:
        raise JbError(rc, f"rectangle {bad.value} does not lie in the image" if bad.value >= 0 else "bad target size or descriptor")


def views_check(desc, views, resize, filter=FILTER_AREA):
    """jb_views_check: can the K views per image of `views` ([[(x, y, w, h[, mirror]), ...], ...]) of the descriptor's
    image be had at the target size (w, h) under `filter`?  Raises JbError otherwise, the text naming the image and the
    view that is to blame when one is."""
    arr, k = _view_array(views)
    n = len(list(views))
    bad = ctypes.c_int(-1)
    rc = lib().jb_views_check(ctypes.byref(desc), arr, n, k, ctypes.byref(_resize_struct(resize, filter)), ctypes.byref(bad))
    if rc != JB_OK:
        raise JbError(rc, f"image {bad.value // k}, view {bad.value % k} cannot be had" if bad.value >= 0 else "bad target size, filter, count or descriptor")


def view_groups_check(desc, views, view_groups):
    """jb_view_groups_check: can the views ([[(x, y, w, h[, mirror]), ... K], ...], group-major within an image) be had in
    the groups [(k, (w, h)[, filter]), ...]?  Raises JbError otherwise, the text naming the image and the view that is to
    blame when one is."""
    arr, k = _view_array(views)
    groups, n_groups = _group_array(view_groups)
    bad = ctypes.c_int(-1)
    rc = lib().jb_view_groups_check(ctypes.byref(desc), arr, len(list(views)), groups, n_groups, ctypes.byref(bad))
    if rc != JB_OK:
        raise JbError(rc, f"image {bad.value // k}, view {bad.value % k} cannot be had" if bad.value >= 0 else "bad groups, target size, filter, count or descriptor")


def color_check(chains):
    """jb_color_check: can the chains ([chain, ...], a chain being None / [(op, value), ...] / a ColorChain) be had?  Raises
    JbError otherwise (.bad_index: the first chain that fails, -1 when none is to blame)."""
    chains = list(chains)
    bad = ctypes.c_int(-1)
    rc = lib().jb_color_check(_chain_array(chains), len(chains), ctypes.byref(bad))
    if rc != JB_OK:
        e = JbError(rc, lib().jb_last_error(None).decode(errors="replace"))
        e.bad_index = bad.value
        raise e


def blur_params(radius):
    """jb_blur_params: Pillow's GaussianBlur radius -> (r, ww, fw), the box radius and the two 8.24 weights of one of its six
    passes.  JbError for a radius that is negative or not finite (-2) or whose box radius is above COLOR_BLUR_BOX_MAX (-9)."""
    r, ww, fw = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().jb_blur_params(float(radius), ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw)))
    return r.value, ww.value, fw.value


def warp_params(op, value, w, h):
    """jb_warp_params: a geometric operation (COLOR_SHEAR_X .. COLOR_ROTATE) on a view of w x h -> (mode, [c0 .. c5]): Pillow's
    path (WARP_SHIFT: xin = x + c2, yin = y + c5; WARP_FIXED: xin = (c2 + y c1 + x c0) >> 16, yin = (c5 + y c4 + x c3) >> 16 in
    int32) and its six integers.  JbError(-2) for another op, a size outside 1..65535, a value that is not finite, a translation
    that is not integral or beyond +-65535; JbError(-9) for a matrix of Pillow's scaling path (a rotation by 180 degrees) or of
    its float path."""
    mode, coef = ctypes.c_int32(), (ctypes.c_int32 * 6)()
    _check(lib().jb_warp_params(int(op), float(value), int(w), int(h), ctypes.byref(mode), coef))
    return mode.value, list(coef)


def color_lut(op, counts):
    """jb_color_lut: the 256-entry table of one channel from its 256 counts (uint32, adding up to less than 2^32), for op =
    COLOR_AUTOCONTRAST (ImageOps.autocontrast, cutoff 0) or COLOR_EQUALIZE (ImageOps.equalize) -> a uint8 array.  The one text
    of the two tables: the device's table kernel compiles it too.  JbError(-2) for another op, another shape, a count that is
    negative or not integral, or counts that add up to 2^32 or more."""
    import numpy as np
    given = np.asarray(counts)
    if given.shape != (256,) or given.dtype.kind not in "iuf":
        raise JbError(-2, "color_lut wants 256 counts")
    exact = [int(c) for c in given.tolist()] if given.dtype.kind != "f" or bool(np.all(np.isfinite(given))) else None
    if exact is None or any(c < 0 for c in exact) or exact != given.tolist() or sum(exact) >= 1 << 32:
        raise JbError(-2, "color_lut wants non-negative integral counts that add up to less than 2^32")
    h = np.array(exact, dtype=np.uint32)
    lut = np.zeros(256, np.uint8)
    _check(lib().jb_color_lut(int(op), _ptr(h), _ptr(lut)))
    return lut


def color_host(image, chain):
    """jb_color_host: the chain on a host [h, w, 3] uint8 array -> a new array.  The CPU statement of the device kernels'
    arithmetic (the same csrc/jb_color_core.h), for tests and for checking a pipeline without a GPU."""
    import numpy as np
    a = np.ascontiguousarray(image, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise JbError(-2, "color_host wants an [h, w, 3] uint8 image")
    out = np.empty_like(a)
    c = ColorChain.make(chain)
    _check(lib().jb_color_host(_ptr(a), a.strides[0], a.shape[1], a.shape[0], ctypes.byref(c), _ptr(out), out.strides[0]))
    return out


def view_groups_bytes(view_groups, fmt=FMT_RGB_U8_HWC):
    """jb_view_groups_bytes: -> ([the byte offset of every group in a file's block], the block's bytes): group 0's outputs,
    then group 1's, ..., tight, in format `fmt` (a format number or an OutputSpec)."""
    groups, n_groups = _group_array(view_groups)
    offsets, total = (ctypes.c_int64 * VIEW_GROUPS_MAX)(), ctypes.c_int64()
    _check(lib().jb_view_groups_bytes(groups, n_groups, fmt.format if isinstance(fmt, OutputSpec) else int(fmt), offsets, ctypes.byref(total)))
    return list(offsets[:n_groups]), total.value


def _resize_struct(resize, filter):
    w, h = resize if resize is not None else (0, 0)
    return Resize(int(w), int(h), int(filter), 0)


def filter_check(desc, resize, filter, roi=None):
    """jb_filter_check: resize_check, and can `filter` take the rectangle (None: the whole image) to the target size
    (w, h)?  Raises JbError otherwise (-2 unknown filter, -7 no target size, -9 more taps than the kernel's cap)."""
    _check(lib().jb_filter_check(ctypes.byref(desc), _ref(_Request(roi=roi).roi), ctypes.byref(_resize_struct(resize, filter))))


def filter_window(desc, resize, filter, roi=None):
    """jb_filter_window: -> (x, y, w, h), the pixels of the frame the filter reads for this request: the rectangle grown
    by the filter's reach, clamped to the frame."""
    win = Roi()
    _check(lib().jb_filter_window(ctypes.byref(desc), _ref(_Request(roi=roi).roi), ctypes.byref(_resize_struct(resize, filter)), ctypes.byref(win)))
    return win.x, win.y, win.width, win.height


def fit_geometry(width, height, resize, fit, roi=None, filter=FILTER_AREA):
    """jb_fit_check: -> ((sx, sy, sw, sh), (ix, iy, iw, ih)) -- the rectangle of the width x height frame that `fit` (None / a
    mode number / a Fit) resamples, and the rectangle of the target resize=(w, h) it lands in; roi: the source (None: the
    whole frame).  What maps a box between a file and its tensor: x_out = ix + (x - sx) * iw / sw.  width, height: of the
    frame the coordinates are in -- entropy_decode(..., headers_only=True) gives a file's, oriented_size the oriented
    one's.  Raises JbError as a decode with these arguments would (-2, -7, -9)."""
    q = _Request(roi=roi)
    f = _fit_struct(fit)
    g = FitGeometry()
    _check(lib().jb_fit_check(ctypes.byref(make_desc(int(width), int(height), 1, 1)), _ref(q.roi), ctypes.byref(_resize_struct(resize, filter)),
                              _ref(f), ctypes.byref(g)))
    return (g.src.x, g.src.y, g.src.width, g.src.height), (g.inner.x, g.inner.y, g.inner.width, g.inner.height)


def _shape_groups(ptr, spec, shapes):
    """"view groups": a file's block at `ptr` as a list of copy-free views, one per group: shapes = [(k, w, h), ...]."""
    fmt = spec.format if spec is not None else FMT_RGB_U8_HWC
    out, at = [], 0
    for k, w, h in shapes:
        out.append(_shape_output(ctypes.c_void_p(ptr + at), w, h, spec, k))
        at += k * output_bytes(w, h, fmt)
    return out


def _shape_output(ptr, w, h, spec, k=0):
    """A copy-free view of one decoded image at `ptr`: [H, W, 3] uint8 (no spec / format 0) or [3, H, W] in the format's
    type.  k > 0 ("views"): the file's k outputs back to back, [k, H, W, 3] or [k, 3, H, W]."""
    lead = (k,) if k else ()
    if spec is None or spec.format == FMT_RGB_U8_HWC:
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(max(k, 1) * w * h * 3,)).reshape(lead + (h, w, 3))
    dt = np.dtype(FMT_DTYPE[spec.format])
    raw = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(max(k, 1) * w * h * 3 * dt.itemsize,))
    return raw.view(dt).reshape(lead + (3, h, w))


def build_library():
    """Compile csrc/ for gfx950 into jpeg_decoder_amd/libjpegblk.so (hipcc cross-compiles
    without a GPU)."""
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc")], check=True, stdout=subprocess.DEVNULL)


def lib_path():
    return _LIB_PATH


_lib = None


def lib():
    """The loaded C-ABI library.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH) and not os.environ.get("JPEGBLK_LIB"):
        # not built yet (fresh checkout): compile it -- building is not a fallback, there is none
        try:
            build_library()
        except Exception as e:  # hipcc missing, compile error ...
            raise ImportError(f"{_LIB_PATH} is missing and could not be built ({e}); run "
                              "`python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback for the block pipeline)") from e
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} is missing (there is no CPU fallback for the block pipeline)")
    # PyTorch bundles its own HIP/HSA runtime with the same sonames as /opt/rocm's; two copies
    # in one process cannot both open the GPU.  Load torch's first (when torch is present) so
    # that libjpegblk.so binds to the runtime torch tensors and streams live in.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(_LIB_PATH)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    pd = ctypes.POINTER(ImageDesc)
    L.jb_abi_version.restype = ctypes.c_int
    L.jb_device_count.restype = ctypes.c_int
    L.jb_geometry_of.argtypes = [pd, ctypes.POINTER(Geometry)]
    L.jb_ctx_create.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(vp)]
    L.jb_ctx_destroy.argtypes = [vp]
    L.jb_ctx_destroy.restype = None
    L.jb_last_error.argtypes = [vp]
    L.jb_last_error.restype = ctypes.c_char_p
    L.jb_ctx_stream.argtypes = [vp]
    L.jb_ctx_stream.restype = vp
    L.jb_ctx_synchronize.argtypes = [vp]
    L.jb_blocks_to_rgb.argtypes = [vp, pd, vp, vp, vp, i64]
    L.jb_submit.argtypes = [vp, pd, vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int)]
    L.jb_wait.argtypes = [vp, ctypes.c_int]
    L.jb_pinned_alloc.argtypes = [ctypes.c_size_t]
    L.jb_pinned_alloc.restype = vp
    L.jb_pinned_alloc_on.argtypes = [ctypes.c_int, ctypes.c_size_t]
    L.jb_pinned_alloc_on.restype = vp
    L.jb_device_numa_node.argtypes = [ctypes.c_int]
    L.jb_ctx_reserve.argtypes = [vp, ctypes.c_size_t, ctypes.c_size_t]
    L.jb_ctx_device.argtypes = [vp]
    L.jb_ctx_device_entropy_images.argtypes = [vp]
    L.jb_ctx_device_entropy_images.restype = ctypes.c_longlong
    L.jb_entropy_decode_device.argtypes = [vp, vp, ctypes.c_size_t, pd, vp, vp, ctypes.c_size_t]
    L.jb_pinned_free.argtypes = [vp]
    L.jb_pinned_free.restype = None
    L.jb_blocks_to_rgb_device.argtypes = [vp, ctypes.POINTER(DeviceBatch), vp]
    L.jb_resolve_qtabs.argtypes = [pd, vp, vp]
    L.jb_kernel_name.argtypes = [pd]
    L.jb_kernel_name.restype = ctypes.c_char_p
    L.jb_ctx_last_front.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    L.jb_flat_front_geometry.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i64]
    L.jb_entropy_decode.argtypes = [vp, ctypes.c_size_t, pd, vp, vp, ctypes.c_size_t]
    L.jb_entropy_decode_mt.argtypes = [vp, ctypes.c_size_t, pd, vp, vp, ctypes.c_size_t, ctypes.c_int]
    L.jb_decode_file.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_decode_memory.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_decode_batch.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32),
                                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
    L.jb_batch_decoder_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.jb_batch_decoder_create_multi.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_size_t,
                                                ctypes.c_size_t, ctypes.POINTER(vp)]
    L.jb_batch_decoder_device_entropy_images.argtypes = [vp]
    L.jb_batch_decoder_device_entropy_images.restype = ctypes.c_longlong
    L.jb_batch_decoder_run.argtypes = [vp] + L.jb_decode_batch.argtypes[1:3] + L.jb_decode_batch.argtypes[4:]
    L.jb_batch_decoder_destroy.argtypes = [vp]
    L.jb_batch_decoder_destroy.restype = None
    L.jb_batch_decoder_submit.argtypes = L.jb_batch_decoder_run.argtypes[:-1] + [ctypes.POINTER(ctypes.c_int)]
    L.jb_batch_decoder_collect.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.jb_poll.argtypes = [vp, ctypes.c_int]
    L.jb_submit_batch.argtypes = [vp, ctypes.POINTER(ImageDesc), ctypes.c_int, vp, vp, vp, ctypes.POINTER(ctypes.c_int)]
    L.jb_batch_decoder_set_arena.argtypes = [vp, ctypes.c_size_t]
    L.jb_batch_decoder_set_device_output.argtypes = [vp, vp, ctypes.c_size_t]
    L.jb_batch_decoder_set_device_output.restype = ctypes.c_int
    L.jb_batch_decoder_set_device_outputs.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int]
    L.jb_batch_decoder_set_device_outputs.restype = ctypes.c_int
    L.jb_free.argtypes = [vp]
    L.jb_free.restype = None
    L.jb_scaled_size.argtypes = [i32, i32, ctypes.c_int, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_blocks_to_rgb_device_scaled.argtypes = [vp, ctypes.POINTER(DeviceBatch), ctypes.c_int, vp]
    L.jb_decode_memory_scaled.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_decode_file_scaled.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_batch_decoder_set_scale.argtypes = [vp, ctypes.c_int]
    ps = ctypes.POINTER(OutputSpec)
    L.jb_output_bytes.argtypes = [i32, i32, ctypes.c_int, ctypes.POINTER(i64)]
    L.jb_output_spec_check.argtypes = [ps, i32, i64]
    L.jb_blocks_to_rgb_device_fmt.argtypes = [vp, ctypes.POINTER(DeviceBatch), ps, vp]
    L.jb_decode_memory_fmt.argtypes = [vp, vp, ctypes.c_size_t, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_decode_file_fmt.argtypes = [vp, ctypes.c_char_p, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_batch_decoder_set_output_format.argtypes = [vp, ps]
    pr = ctypes.POINTER(Roi)
    L.jb_roi_check.argtypes = [pd, pr]
    L.jb_blocks_to_rgb_device_roi.argtypes = [vp, ctypes.POINTER(DeviceBatch), pr, ps, vp]
    L.jb_decode_memory_roi.argtypes = [vp, vp, ctypes.c_size_t, pr, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_decode_file_roi.argtypes = [vp, ctypes.c_char_p, pr, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_batch_decoder_set_roi.argtypes = [vp, pr]
    L.jb_resize_check.argtypes = [pd, pr, i32, i32]
    L.jb_blocks_to_rgb_device_resized.argtypes = [vp, ctypes.POINTER(DeviceBatch), pr, i32, i32, ps, vp]
    L.jb_decode_memory_resized.argtypes = [vp, vp, ctypes.c_size_t, pr, i32, i32, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_decode_file_resized.argtypes = [vp, ctypes.c_char_p, pr, i32, i32, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_batch_decoder_set_resize.argtypes = [vp, i32, i32]
    L.jb_crops_check.argtypes = [pd, pr, ctypes.c_int, i32, i32, ctypes.POINTER(ctypes.c_int)]
    L.jb_blocks_to_rgb_device_crops.argtypes = [vp, ctypes.POINTER(DeviceBatch), pr, i32, i32, ps, vp]
    L.jb_batch_decoder_run_crops.argtypes = L.jb_batch_decoder_run.argtypes[:3] + [pr] + L.jb_batch_decoder_run.argtypes[3:]
    L.jb_batch_decoder_submit_crops.argtypes = L.jb_batch_decoder_submit.argtypes[:3] + [pr] + L.jb_batch_decoder_submit.argtypes[3:]
    prs = ctypes.POINTER(Resize)
    pv = ctypes.POINTER(View)
    L.jb_views_check.argtypes = [pd, pv, ctypes.c_int, ctypes.c_int, prs, ctypes.POINTER(ctypes.c_int)]
    L.jb_blocks_to_rgb_device_views.argtypes = [vp, ctypes.POINTER(DeviceBatch), pv, ctypes.c_int, prs, ps, vp]
    L.jb_batch_decoder_run_views.argtypes = L.jb_batch_decoder_run.argtypes[:3] + [pv, ctypes.c_int] + L.jb_batch_decoder_run.argtypes[3:]
    L.jb_batch_decoder_submit_views.argtypes = L.jb_batch_decoder_submit.argtypes[:3] + [pv, ctypes.c_int] + L.jb_batch_decoder_submit.argtypes[3:]
    pg = ctypes.POINTER(ViewGroup)
    L.jb_view_groups_check.argtypes = [pd, pv, ctypes.c_int, pg, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.jb_view_groups_bytes.argtypes = [pg, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.jb_blocks_to_rgb_device_view_groups.argtypes = [vp, ctypes.POINTER(DeviceBatch), pv, pg, ctypes.POINTER(ViewOutput), ctypes.c_int, ps, vp]
    L.jb_batch_decoder_run_view_groups.argtypes = L.jb_batch_decoder_run.argtypes[:3] + [pv, pg, ctypes.c_int] + L.jb_batch_decoder_run.argtypes[3:]
    L.jb_batch_decoder_submit_view_groups.argtypes = L.jb_batch_decoder_submit.argtypes[:3] + [pv, pg, ctypes.c_int] + L.jb_batch_decoder_submit.argtypes[3:]
    pc = ctypes.POINTER(ColorChain)
    L.jb_color_check.argtypes = [pc, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.jb_color_host.argtypes = [vp, i64, i32, i32, pc, vp, i64]
    L.jb_blur_params.argtypes = [ctypes.c_float, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.jb_color_lut.argtypes = [ctypes.c_int, vp, vp]
    L.jb_warp_params.argtypes = [ctypes.c_int, ctypes.c_float, i32, i32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.jb_color_device.argtypes = [vp, vp, i64, i64, i32, i32, i32, pc, vp, i64, i64, ps, vp]
    L.jb_blocks_to_rgb_device_views_color.argtypes = [vp, ctypes.POINTER(DeviceBatch), pv, ctypes.c_int, prs, pc, ps, vp]
    L.jb_blocks_to_rgb_device_view_groups_color.argtypes = [vp, ctypes.POINTER(DeviceBatch), pv, pg, ctypes.POINTER(ViewOutput), ctypes.c_int, pc, ps, vp]
    L.jb_batch_decoder_run_views_color.argtypes = L.jb_batch_decoder_run.argtypes[:3] + [pv, ctypes.c_int, pc] + L.jb_batch_decoder_run.argtypes[3:]
    L.jb_batch_decoder_submit_views_color.argtypes = L.jb_batch_decoder_submit.argtypes[:3] + [pv, ctypes.c_int, pc] + L.jb_batch_decoder_submit.argtypes[3:]
    L.jb_batch_decoder_run_view_groups_color.argtypes = L.jb_batch_decoder_run.argtypes[:3] + [pv, pg, ctypes.c_int, pc] + L.jb_batch_decoder_run.argtypes[3:]
    L.jb_batch_decoder_submit_view_groups_color.argtypes = L.jb_batch_decoder_submit.argtypes[:3] + [pv, pg, ctypes.c_int, pc] + L.jb_batch_decoder_submit.argtypes[3:]
    L.jb_filter_check.argtypes = [pd, pr, prs]
    L.jb_filter_window.argtypes = [pd, pr, prs, pr]
    L.jb_blocks_to_rgb_device_filtered.argtypes = [vp, ctypes.POINTER(DeviceBatch), pr, prs, ps, vp]
    L.jb_blocks_to_rgb_device_crops_filtered.argtypes = [vp, ctypes.POINTER(DeviceBatch), pr, prs, ps, vp]
    L.jb_decode_memory_filtered.argtypes = [vp, vp, ctypes.c_size_t, pr, prs, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_decode_file_filtered.argtypes = [vp, ctypes.c_char_p, pr, prs, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_batch_decoder_set_filter.argtypes = [vp, ctypes.c_int]
    pf = ctypes.POINTER(Fit)
    L.jb_fit_check.argtypes = [pd, pr, prs, pf, ctypes.POINTER(FitGeometry)]
    L.jb_blocks_to_rgb_device_fit.argtypes = [vp, ctypes.POINTER(DeviceBatch), pr, prs, pf, ps, vp]
    L.jb_decode_memory_fit.argtypes = [vp, vp, ctypes.c_size_t, pr, prs, pf, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_decode_file_fit.argtypes = [vp, ctypes.c_char_p, pr, prs, pf, ps, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_batch_decoder_set_fit.argtypes = [vp, pf]
    L.jb_batch_decoder_set_arithmetic.argtypes = [vp, ctypes.c_int]
    L.jb_ctx_set_arithmetic.argtypes = [vp, ctypes.c_int]
    L.jb_ctx_arithmetic.argtypes = [vp]
    L.jb_ctx_set_orientation.argtypes = [vp, ctypes.c_int]
    L.jb_ctx_orientation.argtypes = [vp]
    L.jb_batch_decoder_set_orientation.argtypes = [vp, ctypes.c_int]
    L.jb_ctx_set_draft.argtypes = [vp, ctypes.c_int]
    L.jb_ctx_draft.argtypes = [vp]
    L.jb_batch_decoder_set_draft.argtypes = [vp, ctypes.c_int]
    L.jb_draft_geometry_of.argtypes = [pd, ctypes.c_int, ctypes.POINTER(DraftGeometry)]
    L.jb_exif_orientation.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    L.jb_oriented_size.argtypes = [i32, i32, ctypes.c_int, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.jb_orient_map_roi.argtypes = [i32, i32, ctypes.c_int, pr, pr]
    L.jb_orient_check.argtypes = [pd, ctypes.c_int, ctypes.c_int, pr]
    L.jb_write_ppm.argtypes = [ctypes.c_char_p, vp, i32, i32, i64]
    L.jb_write_bmp.argtypes = [ctypes.c_char_p, vp, i32, i32, i64]
    if L.jb_abi_version() != 1:
        raise ImportError("libjpegblk.so ABI version mismatch")
    _lib = L
    return L


def make_desc(width, height, hs, vs, qtab_id=(0, 1, 1)):
    d = ImageDesc()
    d.width, d.height, d.hs, d.vs = int(width), int(height), int(hs), int(vs)
    for i in range(3):
        d.qtab_id[i] = int(qtab_id[i])
    d.reserved = 0
    return d


def _check(rc, ctx=None):
    if rc != JB_OK:
        raise JbError(rc, lib().jb_last_error(ctx).decode(errors="replace"))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def geometry_of(desc):
    g = Geometry()
    _check(lib().jb_geometry_of(ctypes.byref(desc), ctypes.byref(g)))
    return g


def flat_front_geometry(hs, vs, linear, mcus_x, mcus_y, n_images, coef_image_stride):
    """jb_flat_front_geometry: may a launch of n_images such images take the 4:4:4 kernel's flat front end?  (no GPU needed)"""
    return bool(lib().jb_flat_front_geometry(hs, vs, int(linear), mcus_x, mcus_y, n_images, coef_image_stride))


def scaled_size(width, height, scale):
    """jb_scaled_size: (ceil(width / scale), ceil(height / scale)) for scale in {1, 2, 4, 8}."""
    w, h = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().jb_scaled_size(int(width), int(height), int(scale), ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


def exif_orientation(jpeg_bytes):
    """jb_exif_orientation: the Exif Orientation tag (1..8) of a JFIF byte string; 1 when it has none or the tag is not
    a SHORT in 1..8.  JbError(-8) when the bytes do not start with SOI."""
    buf = np.frombuffer(jpeg_bytes, dtype=np.uint8)
    o = ctypes.c_int(1)
    if buf.size == 0:
        raise JbError(-8, "no bytes")
    _check(lib().jb_exif_orientation(_ptr(buf), buf.size, ctypes.byref(o)))
    return o.value


def oriented_size(width, height, orientation):
    """jb_oriented_size: (w, h) of the image once the orientation (1..8) is applied: swapped for 5..8."""
    w, h = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().jb_oriented_size(int(width), int(height), int(orientation), ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


def orient_map_roi(width, height, orientation, roi):
    """jb_orient_map_roi: the rectangle (x, y, w, h) of the stored width x height frame that shows as `roi` of the
    oriented one."""
    out = Roi()
    _check(lib().jb_orient_map_roi(int(width), int(height), int(orientation), ctypes.byref(_Request(roi=roi).roi), ctypes.byref(out)))
    return out.x, out.y, out.width, out.height


def draft_geometry(desc, denom):
    """jb_draft_geometry_of: the DraftGeometry of `desc` at draft `denom` (1, 2, 4, 8) -- width x height is the draft
    frame that every output option of a context with that draft then acts on."""
    g = DraftGeometry()
    _check(lib().jb_draft_geometry_of(ctypes.byref(desc), int(denom), ctypes.byref(g)))
    return g


def output_bytes(width, height, fmt=FMT_RGB_U8_HWC):
    """jb_output_bytes: bytes of one width x height image in a format (tight rows and planes)."""
    n = ctypes.c_int64()
    _check(lib().jb_output_bytes(int(width), int(height), int(fmt.format if isinstance(fmt, OutputSpec) else fmt), ctypes.byref(n)))
    return n.value


def resolve_qtabs(desc, qtabs):
    """(uint16 [4,64], desc.qtab_id) -> int32 [3,64], the layout the kernel reads."""
    q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(4, 64)
    out = np.zeros((3, 64), np.int32)
    _check(lib().jb_resolve_qtabs(ctypes.byref(desc), _ptr(q), _ptr(out)))
    return out


def entropy_decode(jpeg_bytes, headers_only=False, n_threads=1):
    """Host front end: JFIF bytes -> (desc, qtabs uint16 [4,64], coef int16 [n,64] or None).
    n_threads > 1 decodes the restart intervals of the image in parallel."""
    buf = np.frombuffer(jpeg_bytes, dtype=np.uint8)
    desc = ImageDesc()
    q = np.zeros((4, 64), np.uint16)
    _check(lib().jb_entropy_decode(_ptr(buf), buf.size, ctypes.byref(desc), _ptr(q), None, 0))
    if headers_only:
        return desc, q, None
    g = geometry_of(desc)
    coef = np.zeros((g.n_coded_blocks, 64), np.int16)
    _check(lib().jb_entropy_decode_mt(_ptr(buf), buf.size, ctypes.byref(desc), _ptr(q), _ptr(coef), coef.nbytes, n_threads))
    return desc, q, coef


class Context:
    """jb_ctx: one device, one stream, a ring of staging slots."""

    def __init__(self, device=0, max_coef_bytes=0, max_rgb_bytes=0, n_slots=2, arithmetic=ARITH_REFERENCE, orientation=ORIENT_STORED,
                 draft=1):
        self._h = ctypes.c_void_p()
        _check(lib().jb_ctx_create(device, max_coef_bytes, max_rgb_bytes, n_slots, ctypes.byref(self._h)))
        try:
            if arithmetic != ARITH_REFERENCE:
                self.set_arithmetic(arithmetic)
            if orientation != ORIENT_STORED:
                self.set_orientation(orientation)
            if draft != 1:
                self.set_draft(draft)
        except JbError:
            self.close()
            raise

    def set_draft(self, draft):
        """jb_ctx_set_draft: 1, or under ARITH_LIBJPEG 2, 4, 8 -- every later call of this context then decodes libjpeg's
        1/2, 1/4 or 1/8 reduced image (Pillow's im.draft(); NOT scale=) and fmt, roi, resize, crops, views, filter and
        fit act on that draft frame: rectangles and sizes are in its coordinates (draft_geometry).  JbError -2 for another
        value, -7 while a submission is in flight; with ARITH_REFERENCE, a scale other than 1 or an orientation other than
        ORIENT_STORED a draft other than 1 is JbError -9 at the call."""
        _check(lib().jb_ctx_set_draft(self._h, int(draft)), self._h)

    @property
    def draft(self):
        return lib().jb_ctx_draft(self._h)

    def set_orientation(self, orientation):
        """jb_ctx_set_orientation: ORIENT_STORED (the pixels as the file stores them), 2..8 (that Exif code, whatever the
        file says) or ORIENT_EXIF (decode_file / decode_memory take the file's own tag; the seam has no file: JbError -7
        there).  Every later call of this context then applies it on the device BEFORE fmt, roi, resize, crops and
        filter, whose rectangles and sizes are the oriented image's.  JbError -2 for a value outside 0..8, -7 while a
        submission is in flight; a scale other than 1 with an orientation other than 1 is JbError -9 at the call."""
        _check(lib().jb_ctx_set_orientation(self._h, int(orientation)), self._h)

    @property
    def orientation(self):
        return lib().jb_ctx_orientation(self._h)

    def set_arithmetic(self, arithmetic):
        """jb_ctx_set_arithmetic: ARITH_REFERENCE, or ARITH_LIBJPEG -- every later call of this context then decodes with
        libjpeg's integer IDCT, fancy upsampling and colour tables: the full-size output is Pillow's
        Image.open(f).convert("RGB") bit for bit, and fmt, roi, resize, crops and filter compose on top of it.  JbError -2
        for an unknown value, -7 while a submission is in flight; a scale other than 1 is then JbError -9 at the call."""
        _check(lib().jb_ctx_set_arithmetic(self._h, int(arithmetic)), self._h)

    @property
    def arithmetic(self):
        return lib().jb_ctx_arithmetic(self._h)

    @classmethod
    def for_image(cls, desc, device=0, n_slots=2):
        g = geometry_of(desc)
        return cls(device, g.coef_bytes, g.rgb_bytes, n_slots)

    def close(self):
        if self._h:
            lib().jb_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def reserve(self, max_coef_bytes, max_rgb_bytes):
        """jb_ctx_reserve: grow (or create) the staging ring."""
        _check(lib().jb_ctx_reserve(self._h, max_coef_bytes, max_rgb_bytes), self._h)

    @property
    def device(self):
        return lib().jb_ctx_device(self._h)

    def last_front(self):
        """jb_ctx_last_front: (JB_FRONT_* of the context's last launch of the tile kernel -- 0 none yet, 1 general, 2 flat --,
        1 if that launch's tiling was linear else 0)."""
        linear = ctypes.c_int(0)
        front = lib().jb_ctx_last_front(self._h, ctypes.byref(linear))
        return front, linear.value

    @property
    def device_entropy_images(self):
        """Images this context decoded with the entropy stage on the device."""
        return lib().jb_ctx_device_entropy_images(self._h)

    def entropy_decode_device(self, jpeg_bytes):
        """jb_entropy_decode_device: JFIF bytes (with restart intervals) -> (desc, qtabs, coef int16
        [n, 64]) with the Huffman stage on the GPU; the coefficients come back through a torch
        tensor (plumbing).  Raises JbError(-9) when the stream is not eligible."""
        import torch
        buf = np.frombuffer(jpeg_bytes, dtype=np.uint8)
        desc, q, _ = entropy_decode(jpeg_bytes, headers_only=True)
        g = geometry_of(desc)
        t = torch.full((g.n_coded_blocks, 64), 0x5a5a, dtype=torch.int16, device=f"cuda:{self.device}")
        torch.cuda.synchronize()
        d2 = ImageDesc()
        q2 = np.zeros((4, 64), np.uint16)
        _check(lib().jb_entropy_decode_device(self._h, _ptr(buf), buf.size, ctypes.byref(d2), _ptr(q2), t.data_ptr(), t.numel() * 2), self._h)
        return d2, q2, t.cpu().numpy()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().jb_ctx_stream(self._h)

    def synchronize(self):
        _check(lib().jb_ctx_synchronize(self._h), self._h)

    # -- the seam, host buffers --------------------------------------------------------------
    def _host_output_size(self, desc):
        """(w, h) of what the host seam writes for `desc` under this context's orientation and draft: the oriented
        frame's, or the draft frame's (the two do not combine: the call answers JbError -9).
        ORIENT_EXIF has no file here: JbError -7, as the C entry points answer, before any buffer is sized."""
        o = self.orientation
        k = self.draft
        if k != 1:
            g = draft_geometry(desc, k)
            return g.width, g.height
        if o == ORIENT_EXIF:
            raise JbError(-7, "ORIENT_EXIF takes the orientation from a file: the host seam has none (set 1..8)")
        return oriented_size(desc.width, desc.height, o)

    def blocks_to_rgb(self, desc, coef, qtabs, stride=None):
        """-> RGB [H, W, 3] of the ORIENTED frame (the context's orientation: [W, H, 3]-shaped for 5..8); stride: bytes
        between the rows of that output, at least 3 * its width."""
        coef = np.ascontiguousarray(coef, dtype=np.int16)
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(4, 64)
        w, h = self._host_output_size(desc)
        stride = stride or 3 * w
        if stride < 3 * w:
            raise JbError(-2, f"stride {stride} < 3 * {w}")
        out = np.zeros((h, stride), np.uint8)
        _check(lib().jb_blocks_to_rgb(self._h, ctypes.byref(desc), _ptr(coef), _ptr(q), _ptr(out), stride), self._h)
        return out[:, :3 * w].reshape(h, w, 3)

    def submit(self, desc, coef, qtabs, out, stride=None):
        """coef / out: numpy arrays that stay alive until wait(ticket).  out and stride are the ORIENTED output's (the
        context's orientation): h rows of `stride` >= 3 * w bytes with (w, h) = oriented_size(desc.width, desc.height,
        orientation); an `out` smaller than that is JbError -2 here, before anything is written."""
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(4, 64)
        w, h = self._host_output_size(desc)
        stride = stride or 3 * w
        if stride < 3 * w or out.nbytes < (h - 1) * stride + 3 * w:
            raise JbError(-2, f"out holds {out.nbytes} bytes, the {w} x {h} output at stride {stride} needs {(h - 1) * stride + 3 * w}")
        t = ctypes.c_int(-1)
        _check(lib().jb_submit(self._h, ctypes.byref(desc), _ptr(coef), _ptr(q), _ptr(out), stride, ctypes.byref(t)), self._h)
        return t.value

    def submit_batch(self, desc, coef, qtabs, out):
        """jb_submit_batch: n images of one geometry in one submission.  coef int16 [n, blocks, 64],
        qtabs uint16 [n, 4, 64], out uint8 [n, H, 3*W] (tight rows) with W x H the ORIENTED frame under the
        context's orientation (JbError -2 for an `out` smaller than that); all C-contiguous and alive until wait()."""
        n = coef.shape[0]
        assert coef.flags.c_contiguous and qtabs.flags.c_contiguous and out.flags.c_contiguous
        assert qtabs.shape == (n, 4, 64) and out.shape[0] == n
        w, h = self._host_output_size(desc)
        if out.nbytes < n * 3 * w * h:
            raise JbError(-2, f"out holds {out.nbytes} bytes, {n} images of {w} x {h} need {n * 3 * w * h}")
        t = ctypes.c_int()
        _check(lib().jb_submit_batch(self._h, ctypes.byref(desc), n, _ptr(coef), _ptr(qtabs), _ptr(out), ctypes.byref(t)), self._h)
        return t.value

    def poll(self, ticket):
        """True once the submission has completed (non-blocking)."""
        rc = lib().jb_poll(self._h, ticket)
        if rc == 1:
            return False
        _check(rc, self._h)
        return True

    def wait(self, ticket):
        _check(lib().jb_wait(self._h, ticket), self._h)

    # -- the seam, device buffers ------------------------------------------------------------
    def blocks_to_rgb_device(self, batch, stream=None, scale=1, fmt=None, roi=None, resize=None, crops=None, filter=FILTER_AREA, views=None,
                             fit=None, view_groups=None, view_outputs=None, colors=None):
        """scale 2, 4, 8: the batch's d_rgb and strides describe images of scaled_size(desc.width, desc.height, scale).
        fmt (an OutputSpec or a format number): planar output -- the batch's rgb_row_stride is then a plane's.
        roi=(x, y, w, h) (with any fmt, not with a scale): the batch's d_rgb and strides describe images of w x h, the
        rectangle of every image.
        resize=(w, h) (with any fmt, with or without roi, not with a scale): the batch's d_rgb and strides describe images
        of w x h, the exact area resize of every image (or of its rectangle).
        crops=[(x, y, w, h), ...] with resize=(w, h) (with any fmt, not with roi or a scale): one rectangle per image of the
        batch, each resized to w x h (jb_blocks_to_rgb_device_crops); the list is read before the call returns.
        filter=FILTER_BILINEAR / FILTER_BICUBIC with resize= (with or without roi or crops): Pillow's 8-bit resampling in
        the area filter's place (jb_blocks_to_rgb_device_filtered / _crops_filtered).
        views=[[(x, y, w, h[, mirror]), ... K], ... N] with resize=(w, h) (any fmt and filter; not with roi, crops or a scale): K
        rectangles per image, each resized to w x h and then mirrored left-right when its fifth field is true, from ONE
        pixel launch per image (jb_blocks_to_rgb_device_views).  batch.d_rgb and its strides describe n_images * K
        outputs; output i * K + v is view v of image i.
        fit=Fit.pad(fill, anchor) / Fit.cover(anchor) / a mode number with resize=(w, h) (any fmt, roi and filter; not with crops
        or views): the source keeps its aspect ratio -- scaled to fit inside the target with the rest filled, or the largest
        centred rectangle of the target's aspect ratio resized (jb_blocks_to_rgb_device_fit).  None / FIT_STRETCH: as before.
        view_groups=[(k, (w, h)[, filter]), ... G] with views= and view_outputs=[(d_out, image_stride, view_stride, row_stride[,
        plane_stride]) or ViewOutput, ... G] (any fmt, whose plane_stride must be 0; not with resize, filter, roi, crops, fit or a
        scale): the K = sum of k views of an image fall into G groups, group-major, each with its own target size and filter, all
        from ONE pixel launch per image (jb_blocks_to_rgb_device_view_groups); batch.d_rgb and its strides are not read.
        colors=[[chain, ... K], ... N] with views= (and with view_groups=): chain (i, v) -- None / [] (the identity) or [(COLOR_*,
        value), ...], at most 8 operations; at most COLOR_STATS_MAX statistics operations (COLOR_CONTRAST, COLOR_AUTOCONTRAST,
        COLOR_EQUALIZE), one of them a contrast; one neighbourhood operation (COLOR_BLUR or COLOR_SHARPNESS) with no statistics
        operation behind it -- is applied to the uint8 pixels of view v of image i, mirror included, in front of the output
        format: Pillow's ImageEnhance (Brightness, Contrast, Color, Sharpness: a blend against ImageFilter.SMOOTH) / convert /
        ImageOps.solarize / posterize / invert / autocontrast / equalize / ImageFilter.GaussianBlur bit for bit
        (jb_blocks_to_rgb_device_views_color / _view_groups_color).  Without views ValueError.
        Each is the entry point of that suffix (_ROUTES)."""
        request = _Request(scale, fmt, roi, resize, crops, filter, views, fit, view_groups, view_outputs, colors)
        if request.groups is not None and request.outputs is None:
            raise JbError(-1, "view groups want view_outputs")
        if request.crops is not None and request.n_crops != batch.n_images:
            raise JbError(-2, f"{request.n_crops} rectangles (crops) for {batch.n_images} images")
        if request.views is not None and request.n_view_rows != batch.n_images:
            raise JbError(-2, f"{request.n_view_rows} rows of views for {batch.n_images} images")
        route, tail = request.routed()
        _check(getattr(lib(), _ROUTES[route][_DEVICE])(self._h, ctypes.byref(batch), *tail, stream), self._h)

    def color_device(self, d_in, in_row_stride, in_image_stride, width, height, n_images, chains, d_out, out_row_stride, out_image_stride,
                     fmt=None, stream=None):
        """jb_color_device: chain i ([chain, ...], n_images of them) on device image i of n_images interleaved uint8 images of
        width x height at the device address d_in, written in format fmt (None: interleaved uint8) at d_out; the strides are
        bytes, as a batch's d_rgb is described (out_row_stride: a plane's rows when planar).  Launches on `stream`."""
        chains = list(chains)
        if len(chains) != n_images:
            raise JbError(-2, f"{len(chains)} chains for {n_images} images")
        spec = fmt if fmt is None or isinstance(fmt, OutputSpec) else OutputSpec.make(fmt)
        _check(lib().jb_color_device(self._h, ctypes.c_void_p(int(d_in)), in_row_stride, in_image_stride, width, height, n_images,
                                     _chain_array(chains), ctypes.c_void_p(int(d_out)), out_row_stride, out_image_stride, _ref(spec), stream),
               self._h)

    # -- decode(path) -> RGB -----------------------------------------------------------------
    def _decode(self, family, lead, request):
        """One decode(bytes) call: the family's entry point of the request's route over (context, the family's leading
        arguments, the route's, the three outputs) -> a copy of the image, its malloc'ed buffer released."""
        route, tail = request.routed()
        p, w, h = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32()
        _check(getattr(lib(), _ROUTES[route][family])(self._h, *lead, *tail, ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)), self._h)
        try:
            return _shape_output(p, w.value, h.value, request.spec if route != "scaled" else None).copy()
        finally:
            lib().jb_free(p)

    def decode_file(self, path, scale=1, fmt=None, roi=None, resize=None, filter=FILTER_AREA, fit=None):
        """-> RGB [H, W, 3]; scale 2, 4, 8: the area-reduced image; fmt (OutputSpec or format number): [3, H, W] in the
        format's type for the planar formats; roi=(x, y, w, h) (with any fmt, not with a scale): that rectangle of the
        image; resize=(w, h) (with any fmt, with or without roi, not with a scale): the image, or its rectangle, at w x h;
        filter (with resize): FILTER_AREA, or FILTER_BILINEAR / FILTER_BICUBIC for Pillow's 8-bit resampling;
        fit (with resize): Fit.pad(...) / Fit.cover(...) keep the aspect ratio, the output is still w x h.
        Each is jb_decode_file's variant of that suffix (_ROUTES)."""
        request = _Request(scale, fmt, roi, resize, filter=filter, fit=fit)
        return self._decode(_FILE, (os.fsencode(path),), request)

    def decode_memory(self, jpeg_bytes, scale=1, fmt=None, roi=None, resize=None, filter=FILTER_AREA, fit=None):
        """jb_decode_memory: a JFIF byte string -> RGB [H, W, 3] (front end + device seam); scale, fmt, roi, resize,
        filter, fit: as decode_file."""
        buf = np.frombuffer(jpeg_bytes, dtype=np.uint8)
        return self._decode(_MEMORY, (_ptr(buf), buf.size), _Request(scale, fmt, roi, resize, filter=filter, fit=fit))


def _batch_args(paths):
    """The argument arrays of one batch call over `paths`, as the ticket of BatchDecoder.submit holds them."""
    n = len(paths)
    return {"n": n, "paths": (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths]), "rgb": (ctypes.c_void_p * n)(),
            "w": (ctypes.c_int32 * n)(), "h": (ctypes.c_int32 * n)(), "st": (ctypes.c_int * n)(), "id": ctypes.c_int(-1), "k": 0, "groups": None}


def _batch_times(times, rc):
    """The times dict of a batch call: its four times, its status and, when that is not 0, the library's error text."""
    return {"wall_s": times[0], "entropy_s": times[1], "device_s": times[2], "read_s": times[3], "rc": rc,
            "error": lib().jb_last_error(None).decode(errors="replace") if rc else ""}


def _harvest(n, rgb, w, h, st, fmt, keep_pixels, on_image, arena, device_out, k=0, groups=None):
    """The results of a finished batch, without the times: (device pointers (int, 0 = failed), (width, height) per image,
    statuses) with device output, else (arrays / (width, height) without keep_pixels / None = failed, statuses).  Host
    images cost at most one view and one copy each; a malloc'ed one (no arena: arena images belong to the decoder) is
    released here.  Afterwards rgb[] is all NULL: every pointer was released or handed out, none can be harvested twice.
    groups ("view groups": [(k, w, h), ...]): a file's entry is a LIST of G arrays [k, ...], its block taken apart."""
    if device_out:
        out = ([int(rgb[i] or 0) for i in range(n)], [(w[i], h[i]) for i in range(n)])
    else:
        imgs = []
        for i in range(n):
            if rgb[i]:
                if on_image is not None or keep_pixels:
                    view = _shape_groups(rgb[i], fmt, groups) if groups else _shape_output(rgb[i], w[i], h[i], fmt, k)
                    if on_image is not None:
                        on_image(i, view)
                imgs.append(([v.copy() for v in view] if groups else view.copy()) if keep_pixels else (w[i], h[i]))
                if not arena:
                    lib().jb_free(rgb[i])
            else:
                imgs.append(None)
        out = (imgs,)
    ctypes.memset(rgb, 0, ctypes.sizeof(rgb))
    return out + (list(st),)


def _colors_want_views(colors, views):
    if colors is not None and views is None:
        raise ValueError("colors want views (a K = 1 views= call covers a plain one)")


def _batch_route(a, crops, views, view_groups, colors):
    """The batch counterpart of _ROUTES: what a run or a submission over the arrays `a` (_batch_args) is asked for per file ->
    (the suffix of jb_batch_decoder_run / jb_batch_decoder_submit, its arguments between the count and the outputs); a["k"] and
    a["groups"] become the harvest's hints.  JbError / ValueError for what cannot be combined."""
    _colors_want_views(colors, views)
    if view_groups is not None:
        if crops is not None:
            raise JbError(-9, "view groups cannot be combined with per-image rectangles (crops)")
        if views is None:
            raise JbError(-7, "view groups want views")
        groups, n_groups = _group_array(view_groups)
        arr, a["k"] = _view_array(views, a["n"])
        if a["n"] and a["k"] != sum(g.n_views for g in groups[:n_groups]):
            raise JbError(-2, "view groups: every file wants as many views as the groups count")
        a["groups"] = [(g.n_views, g.rs.out_w, g.rs.out_h) for g in groups[:n_groups]]
        suffix, extra = "_view_groups", [arr, groups, n_groups]
    elif views is not None:
        if crops is not None:
            raise JbError(-9, "views cannot be combined with per-image rectangles (crops)")
        arr, a["k"] = _view_array(views, a["n"])
        suffix, extra = "_views", [arr, a["k"]]
    elif crops is not None:
        return "_crops", [_crop_array(crops, a["n"])]
    else:
        return "", []
    if colors is not None:
        return suffix + "_color", extra + [_color_array(colors, a["n"], a["k"])]
    return suffix, extra


class BatchDecoder:
    """jb_batch_decoder: n_threads host lanes (pinned buffers each) feeding one shared context per
    device, reusable.  devices=[...] (jb_batch_decoder_create_multi): one decoder over several
    devices, file i -> devices[i % len(devices)], the host threads split evenly.  scale 2, 4, 8
    (jb_batch_decoder_set_scale): every image comes out area-reduced.  fmt (an OutputSpec or a format number;
    jb_batch_decoder_set_output_format): every image comes out in that format, [3, H, W] for the planar ones.
    roi=(x, y, w, h) (jb_batch_decoder_set_roi; with any fmt, not with a scale): every image comes out as that rectangle of
    itself, so files of different sizes give outputs of one size.  resize=(w, h) (jb_batch_decoder_set_resize; with any
    fmt, with or without roi, not with a scale): every image, or its rectangle, comes out at w x h, an exact area resize
    on the device, so files of any size and layout give outputs of one size.  filter (jb_batch_decoder_set_filter; with
    resize): FILTER_BILINEAR / FILTER_BICUBIC put Pillow's 8-bit resampling in the area filter's place, for the target
    size and for the per-image rectangles of run(crops=) alike.  arithmetic (jb_batch_decoder_set_arithmetic):
    ARITH_LIBJPEG decodes every file as libjpeg does, bit for bit (not with a scale).  orientation
    (jb_batch_decoder_set_orientation): ORIENT_EXIF applies every file's own Exif tag, 2..8 that code to every file, in
    front of every other option: sizes, roi and crops are then the oriented image's (not with a scale).  fit
    (jb_batch_decoder_set_fit; with resize): Fit.pad(...) letterboxes every file into the target, Fit.cover(...) cuts the
    largest centred rectangle of the target's aspect ratio; not with run(crops=) or run(views=).  draft
    (jb_batch_decoder_set_draft; with ARITH_LIBJPEG): 2, 4, 8 decode every file to libjpeg's reduced image, Pillow's draft,
    in front of every other option."""

    def __init__(self, n_threads=8, device=0, max_coef_bytes=0, max_rgb_bytes=0, arena_bytes=0, devices=None, scale=1, fmt=None,
                 roi=None, resize=None, filter=FILTER_AREA, arithmetic=ARITH_REFERENCE, orientation=ORIENT_STORED, fit=None, draft=1):
        _Request(scale, fmt, roi, resize, filter=filter, fit=fit)   # (roi or resize with a scale: JbError(-9) before anything is created)
        self._h = ctypes.c_void_p()
        if devices is not None:
            ids = (ctypes.c_int * len(devices))(*devices)
            _check(lib().jb_batch_decoder_create_multi(ids, len(devices), n_threads, max_coef_bytes, max_rgb_bytes, ctypes.byref(self._h)))
        else:
            _check(lib().jb_batch_decoder_create(device, n_threads, max_coef_bytes, max_rgb_bytes, ctypes.byref(self._h)))
        self._arena = False
        self._device_out = False
        self._flights = {}
        self._fmt = None
        self._device = devices[0] if devices else device
        if arena_bytes:
            _check(lib().jb_batch_decoder_set_arena(self._h, arena_bytes))
            self._arena = True
        try:
            if scale != 1:
                self.set_scale(scale)
            if fmt is not None:
                self.set_output_format(fmt)
            if roi is not None:
                self.set_roi(roi)
            if resize is not None:
                self.set_resize(resize)
            if filter != FILTER_AREA:
                self.set_filter(filter)
            if arithmetic != ARITH_REFERENCE:
                self.set_arithmetic(arithmetic)
            if orientation != ORIENT_STORED:
                self.set_orientation(orientation)
            if fit is not None:
                self.set_fit(fit)
            if draft != 1:
                self.set_draft(draft)
        except JbError:
            self.close()
            raise

    def set_orientation(self, orientation):
        """jb_batch_decoder_set_orientation: ORIENT_STORED, ORIENT_EXIF or 2..8 for later runs and submissions (JbError
        -7 while a batch is in flight, -2 for a value outside 0..8, -9 for any value but ORIENT_STORED while the
        decoder's scale is not 1)."""
        _check(lib().jb_batch_decoder_set_orientation(self._h, int(orientation)))

    def set_output_format(self, fmt):
        """jb_batch_decoder_set_output_format: the format of later runs and submissions (JbError -7 while a batch is
        in flight, -9 when the decoder's scale is not 1)."""
        spec = _Request(fmt=fmt).spec
        _check(lib().jb_batch_decoder_set_output_format(self._h, ctypes.byref(spec)))
        self._fmt = spec

    def set_roi(self, roi):
        """jb_batch_decoder_set_roi: one rectangle (x, y, w, h) for every image of later runs and submissions; None:
        whole images again (JbError -7 while a batch is in flight, -9 when the decoder's scale is not 1).  A file the
        rectangle does not fit in gets status -2 and the batch goes on."""
        _check(lib().jb_batch_decoder_set_roi(self._h, _ref(_Request(roi=roi).roi)))

    def set_resize(self, resize):
        """jb_batch_decoder_set_resize: one output size (w, h) for every image of later runs and submissions; None or
        (0, 0): the images' own sizes again (JbError -7 while a batch is in flight, -9 when the decoder's scale is not 1)."""
        w, h = _Request(resize=resize).target or (0, 0)
        _check(lib().jb_batch_decoder_set_resize(self._h, w, h))

    def set_filter(self, filter):
        """jb_batch_decoder_set_filter: the resampling filter (FILTER_*) of later runs and submissions, for the target size
        and for per-image rectangles alike; kept, and idle, while no target size is set (JbError -7 while a batch is in
        flight, -2 for an unknown filter)."""
        _check(lib().jb_batch_decoder_set_filter(self._h, int(filter)))

    def set_fit(self, fit):
        """jb_batch_decoder_set_fit: the fit (None / a mode number / a Fit) of later runs and submissions, for the target
        size; None or FIT_STRETCH: stretch again.  Kept while no target size is set: the files of such a run get status
        -7 (JbError -7 while a batch is in flight, -2 for an unknown mode or anchor).  While a mode other than FIT_STRETCH
        is set, run(crops=) and run(views=) are refused with -9."""
        if fit is not None and not isinstance(fit, Fit):
            fit = Fit(int(fit), FIT_CENTER, (ctypes.c_uint8 * 3)(0, 0, 0), 0, 0)
        _check(lib().jb_batch_decoder_set_fit(self._h, _ref(fit)))

    def set_draft(self, draft):
        """jb_batch_decoder_set_draft: 1, 2, 4 or 8 for later runs and submissions -- under ARITH_LIBJPEG every file then
        decodes to libjpeg's reduced image (Pillow's draft), and sizes, roi, crops and views are that draft frame's
        (JbError -7 while a batch is in flight, -2 for another value, -9 for a value other than 1 without ARITH_LIBJPEG,
        with a scale other than 1 or an orientation other than ORIENT_STORED)."""
        _check(lib().jb_batch_decoder_set_draft(self._h, int(draft)))

    def set_arithmetic(self, arithmetic):
        """jb_batch_decoder_set_arithmetic: ARITH_REFERENCE or ARITH_LIBJPEG for later runs and submissions (JbError -7
        while a batch is in flight, -2 for an unknown value, -9 for ARITH_LIBJPEG while the decoder's scale is not 1)."""
        _check(lib().jb_batch_decoder_set_arithmetic(self._h, int(arithmetic)))

    def set_scale(self, scale):
        """jb_batch_decoder_set_scale: output at 1/scale for later runs and submissions (JbError -7 while a batch
        is in flight, -9 while a planar format, a rectangle or a target size is set, or under ARITH_LIBJPEG)."""
        _check(lib().jb_batch_decoder_set_scale(self._h, scale))

    @property
    def device_entropy_images(self):
        return lib().jb_batch_decoder_device_entropy_images(self._h)

    def _run(self, paths, keep_pixels, on_image, crops=None, views=None, view_groups=None, colors=None):
        a = _batch_args(paths)
        suffix, extra = _batch_route(a, crops, views, view_groups, colors)
        times = (ctypes.c_double * 4)()
        rc = getattr(lib(), "jb_batch_decoder_run" + suffix)(self._h, a["paths"], a["n"], *extra, a["rgb"], a["w"], a["h"], a["st"], times)
        return self._results(a, _batch_times(times, rc), keep_pixels, on_image)

    def _results(self, a, t, keep_pixels, on_image):
        return _harvest(a["n"], a["rgb"], a["w"], a["h"], a["st"], self._fmt, keep_pixels, on_image, self._arena, self._device_out,
                        a.get("k", 0), a.get("groups")) + (t,)

    def run(self, paths, keep_pixels=True, on_image=None, crops=None, views=None, view_groups=None, colors=None):
        """-> what decode_batch returns, in the decoder's format.  crops=[(x, y, w, h), ...] (jb_batch_decoder_run_crops; a
        target size must be set, a rectangle for every image must not: rc -7 in the times): crops[i] is the rectangle of
        paths[i], in pixels of that file, and every image comes out as its rectangle at the target size; a file its
        rectangle does not fit in gets status -2 and the batch goes on.  JbError(-2) when len(crops) != len(paths).
        views=[[(x, y, w, h[, mirror]), ... K], ...] (jb_batch_decoder_run_views; a target size must be set, rc -7, a scale or
        a rectangle for every image must not, rc -9): views[i] are the K views of paths[i], and the file's entry is ONE
        array [K, ...] in the decoder's format -- the file is decoded once.  A file one of whose views does not fit gets
        status -2.  JbError(-2) for rows of unequal length or len(views) != len(paths).
        view_groups=[(k, (w, h)[, filter]), ... G] with views= (jb_batch_decoder_run_view_groups; the decoder's own target size
        and filter are not read; a scale, a rectangle for every image or a fit must not be set, rc -9): the K = sum of k views
        of a file fall into G groups, group-major, each with its own target size and filter, and the file's entry is a LIST of
        G arrays [k_g, ...] -- the file is still decoded once.
        colors=[[chain, ... K], ...] with views= (jb_batch_decoder_run_views_color / _run_view_groups_color): colors[i][v] --
        None / [] or [(COLOR_*, value), ...] -- is applied to view v of paths[i] on its uint8 pixels, mirror included, in front of
        the decoder's format (Context.blocks_to_rgb_device has the definition).  A bad chain refuses the whole call (the
        rc in the times); without views ValueError; another shape than the views' JbError(-2)."""
        _colors_want_views(colors, views)
        assert not self._device_out, "device output is set: use run_to_device"
        return self._run(paths, keep_pixels, on_image, crops, views, view_groups, colors)

    def set_device_output(self, d_base, nbytes):
        """jb_batch_decoder_set_device_output: decoded images stay in the caller's DEVICE memory
        [d_base, d_base + nbytes) (e.g. a torch uint8 CUDA tensor's data_ptr()); (0, 0) = host output again."""
        _check(lib().jb_batch_decoder_set_device_output(self._h, ctypes.c_void_p(d_base or None), nbytes))
        self._arena = bool(d_base)
        self._device_out = bool(d_base)

    def set_device_outputs(self, regions):
        """jb_batch_decoder_set_device_outputs: [(device pointer, bytes), ...], one per listed device of a
        multi-device decoder; [] = host output again."""
        n = len(regions)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[r[0] for r in regions])
        sizes = (ctypes.c_size_t * max(n, 1))(*[r[1] for r in regions])
        _check(lib().jb_batch_decoder_set_device_outputs(self._h, ptrs, sizes, n))
        self._arena = self._device_out = n > 0

    def run_to_device(self, paths, crops=None, views=None, view_groups=None, colors=None):
        """After set_device_output: -> (device pointers (int, 0 = failed), (width, height) per image, statuses, times).
        crops: as for run().  views: as for run() -- a file's pointer is that of its K outputs, back to back, tight.
        view_groups: as for run() -- a file's pointer is that of its block (view_groups_bytes has the layout).
        colors: as for run()."""
        _colors_want_views(colors, views)
        assert self._device_out, "call set_device_output first"
        return self._run(paths, False, None, crops, views, view_groups, colors)

    def run_to_tensor(self, paths, out, crops=None, views=None, view_groups=None, colors=None):
        """Decode files of ONE size (or, with a rectangle set, of any size the rectangle fits in: out is then
        [N, 3, h, w] of the rectangle; with a target size set, of any size: out is [N, 3, h, w] of the target) straight into a caller-supplied CUDA tensor through the device-output route:
        out is [N, 3, H, W] (planar formats; [N, H, W, 3] for format 0), contiguous, of the decoder's format's dtype, on
        the decoder's device, N = len(paths).  -> (out, statuses, times).  An image whose size does not match out (or
        that fails to decode) gets a non-zero status (JB_ERR_GEOMETRY = -2 for the size) and its slice of out is left
        as it was.  The decoder's device-output setting is replaced for the call and cleared afterwards.
        crops: as for run() -- the random-resized-crop of a batch straight into the model's input tensor.
        views: as for run(); out is then [N, K, 3, h, w] ([N, K, h, w, 3] for format 0).
        view_groups: as for run(); out is then a LIST of G contiguous tensors [N, K_g, 3, h_g, w_g] ([N, K_g, h_g, w_g, 3] for
        format 0), and is returned as it came.
        colors: as for run() -- the colour jitter of every view on the way into the model's input tensor."""
        _colors_want_views(colors, views)
        import torch
        if view_groups is not None:
            return self._run_to_tensors(paths, out, views, view_groups, colors)
        if views is not None:
            views = [list(r) for r in views]
            k = _view_array(views, len(paths))[1]
            lead = (len(paths), k)
            if out.dim() != 5 or tuple(out.shape[:2]) != lead or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous CUDA tensor [{lead[0]}, {lead[1]}, 3, H, W] ([N, K, H, W, 3] for format 0)")
            flat, st, t = self._run_to_tensor(paths, out.view((-1,) + tuple(out.shape[2:])), None, views, k, colors)
            return out, st, t
        return self._run_to_tensor(paths, out, crops, None, 1)

    def _run_to_scratch(self, paths, per, device, crops, views, view_groups, colors):
        """run_to_device into a scratch region of `per` bytes per file -> (scratch, its address, pointers, sizes, statuses, times).
        The decoder places images group by group (a group of one thread's files back to back, groups on 256-byte steps of
        the region, in the order the threads get there): they land here in their final format, and the caller's one
        device-to-device copy per image puts them in order."""
        import torch
        n = len(paths)
        scratch = torch.empty(n * per + 256 * (n + 1), dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)
        self.set_device_output(scratch.data_ptr(), scratch.numel())
        try:
            ptrs, sizes, st, t = self.run_to_device(paths, crops, views, view_groups, colors)
        finally:
            self.set_device_output(0, 0)
        return scratch, scratch.data_ptr(), ptrs, sizes, list(st), t

    def _run_to_tensors(self, paths, outs, views, view_groups, colors=None):
        """run_to_tensor with view groups: the files' blocks land in a scratch region, one copy per file and group sorts them"""
        import torch
        spec = self._fmt
        fmt = spec.format if spec is not None else FMT_RGB_U8_HWC
        planar = fmt != FMT_RGB_U8_HWC
        dt = {np.uint8: torch.uint8, np.float32: torch.float32, np.float16: torch.float16}[FMT_DTYPE[fmt]]
        n = len(paths)
        groups, n_groups = _group_array(view_groups)
        offsets, per = view_groups_bytes(view_groups, fmt)
        outs = list(outs)
        if len(outs) != n_groups:
            raise ValueError(f"{len(outs)} tensors for {n_groups} groups")
        for g, out in zip(groups[:n_groups], outs):
            want = (n, g.n_views, 3, g.rs.out_h, g.rs.out_w) if planar else (n, g.n_views, g.rs.out_h, g.rs.out_w, 3)
            if not (out.is_cuda and out.is_contiguous() and out.dtype == dt and tuple(out.shape) == want):
                raise ValueError(f"a group's tensor must be a contiguous CUDA tensor {list(want)} of {dt}")
            if out.device.index != self._device:
                raise ValueError(f"out is on {out.device}, the decoder on device {self._device}")
        scratch, base, ptrs, sizes, st, t = self._run_to_scratch(paths, per, outs[0].device, None, views, view_groups, colors)
        for g, out in enumerate(outs):
            flat = out.view(n, -1).view(torch.uint8) if out.dtype != torch.uint8 else out.view(n, -1)   # (a row per FILE)
            for i in range(n):
                if st[i] == JB_OK and ptrs[i]:
                    off = ptrs[i] - base + offsets[g]
                    flat[i].copy_(scratch[off:off + flat.shape[1]])
        torch.cuda.synchronize(outs[0].device)
        return outs, st, t

    def _run_to_tensor(self, paths, out, crops, views, k, colors=None):
        """run_to_tensor over out = [N * k, ...]: file i's k outputs are out[i * k : (i + 1) * k]."""
        import torch
        spec = self._fmt
        planar = spec is not None and spec.format != FMT_RGB_U8_HWC
        dt = {np.uint8: torch.uint8, np.float32: torch.float32, np.float16: torch.float16}[FMT_DTYPE[spec.format] if spec is not None else np.uint8]
        n = len(paths)
        if not (out.is_cuda and out.is_contiguous() and out.dtype == dt and out.dim() == 4 and out.shape[0] == n * k and
                out.shape[1 if planar else 3] == 3):
            raise ValueError(f"out must be a contiguous CUDA tensor [{n}, 3, H, W] ([N, H, W, 3] for format 0) of {dt}")
        if out.device.index != self._device:
            raise ValueError(f"out is on {out.device}, the decoder on device {self._device}")
        H, W = (out.shape[2], out.shape[3]) if planar else (out.shape[1], out.shape[2])
        per = output_bytes(W, H, spec.format if spec is not None else FMT_RGB_U8_HWC) * k   # (a file's k outputs)
        assert per == out[0].numel() * out.element_size() * k
        scratch, base, ptrs, sizes, st, t = self._run_to_scratch(paths, per, out.device, crops, views, None, colors)
        flat = out.view(n, -1).view(torch.uint8) if out.dtype != torch.uint8 else out.view(n, -1)   # (a row per FILE)
        for i in range(n):
            if st[i] != JB_OK or not ptrs[i]:
                continue
            if sizes[i] != (W, H):
                st[i] = -2   # JB_ERR_GEOMETRY: not the size of `out`
                continue
            off = ptrs[i] - base
            flat[i].copy_(scratch[off:off + per])
        torch.cuda.synchronize(out.device)
        return out, st, t

    # -- batches in a stream (jb_batch_decoder_submit / _collect): two in flight -----------------
    def submit(self, paths, crops=None, views=None, view_groups=None, colors=None):
        """-> a ticket (keeps the batch's arrays alive); the batch runs while the caller prepares the next one.
        crops: as for run() (jb_batch_decoder_submit_crops, which copies them; a refusal is a JbError here).
        views: as for run() (jb_batch_decoder_submit_views, which copies them).
        view_groups: as for run() (jb_batch_decoder_submit_view_groups, which copies views and groups).
        colors: as for run() (the _color variants, which copy the chains too; a bad chain is a JbError here)."""
        t = _batch_args(paths)
        suffix, extra = _batch_route(t, crops, views, view_groups, colors)
        _check(getattr(lib(), "jb_batch_decoder_submit" + suffix)(self._h, t["paths"], t["n"], *extra, t["rgb"], t["w"], t["h"], t["st"],
                                                                 ctypes.byref(t["id"])))
        # the library writes into these arrays until the batch is collected (or the decoder destroyed): the decoder
        # object holds them as well, so a ticket the caller drops cannot free them under a running batch
        self._flights[t["id"].value] = t
        return t

    def collect(self, ticket, keep_pixels=True, on_image=None):
        """-> what run() returns (host output: arrays / None; with an arena the pixels are views' copies), or, with
        device output set, what run_to_device() returns.  A ticket that is not in flight (collected before, or unknown)
        gives rc -7 in the times and no image: its pointers are stale, none is read or released."""
        times = (ctypes.c_double * 4)()
        rc = lib().jb_batch_decoder_collect(self._h, ticket["id"], times)
        if rc == -7:   # (JB_ERR_STATE: no such batch -- nothing was collected)
            ticket = dict(ticket, rgb=(ctypes.c_void_p * ticket["n"])())
        else:
            self._flights.pop(ticket["id"].value, None)
        return self._results(ticket, _batch_times(times, rc), keep_pixels, on_image)

    def close(self):
        if self._h:
            lib().jb_batch_decoder_destroy(self._h)   # (waits for batches still in flight)
            self._h = ctypes.c_void_p()
            self._flights.clear()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def decode_batch(paths, n_threads=8, device=0, keep_pixels=True, on_image=None, scale=1):
    """jb_decode_batch: -> (list of uint8 [H,W,3] arrays or None, statuses, times dict).
    on_image(i, view): called with a no-copy [H,W,3] view of every decoded image before its buffer
    is released (checks over batches too large to keep).  scale 2, 4, 8: through a temporary
    BatchDecoder with set_scale(scale)."""
    if scale != 1:
        if n_threads > len(paths) > 0:
            n_threads = len(paths)
        with BatchDecoder(n_threads=n_threads, device=device, scale=scale) as d:
            return d.run(paths, keep_pixels=keep_pixels, on_image=on_image)
    a = _batch_args(paths)
    times = (ctypes.c_double * 4)()
    rc = lib().jb_decode_batch(device, a["paths"], a["n"], n_threads, a["rgb"], a["w"], a["h"], a["st"], times)
    return _harvest(a["n"], a["rgb"], a["w"], a["h"], a["st"], None, keep_pixels, on_image, False, False) + (_batch_times(times, rc),)


def torch_batch(desc, n_images, coef_t, qtabs_t, rgb_t, rgb_row_stride=None, shared_qtabs=True, scale=1, fmt=None, roi=None,
                resize=None, filter=FILTER_AREA, fit=None):
    """DeviceBatch over torch CUDA tensors (plumbing): coef_t int16 [n_images, n_blocks, 64],
    qtabs_t int32 [3,64] (shared) or [n_images,3,64], rgb_t uint8 [n_images, H, row_stride].
    scale 2, 4, 8: rgb_t holds the reduced images, [n_images, ceil(H/scale), row_stride], for
    Context.blocks_to_rgb_device(..., scale=scale).
    fmt (a planar OutputSpec / format number, for Context.blocks_to_rgb_device(..., fmt=)): rgb_t is
    [n_images, 3, H, W'] in the format's dtype, W' >= W; strides are taken from the tensor (in bytes) and, when fmt is an
    OutputSpec, its plane_stride is set from rgb_t.stride(1).
    roi=(x, y, w, h) (for Context.blocks_to_rgb_device(..., roi=), with any fmt, not with a scale): rgb_t holds images of
    the rectangle's size, w x h, instead of desc's.
    resize=(w, h) (for Context.blocks_to_rgb_device(..., resize=), with any fmt and roi, not with a scale): rgb_t holds
    images of w x h; filter and fit (for Context.blocks_to_rgb_device(..., filter=, fit=)) change no size."""
    q = _Request(scale, fmt, roi, resize, filter=filter, fit=fit)
    out_w, out_h = q.target if q.target is not None else (q.roi.width, q.roi.height) if q.roi is not None else (desc.width, desc.height)
    if q.spec is not None and q.spec.format != FMT_RGB_U8_HWC:
        assert scale == 1, "an output format cannot be combined with a scale"
        es = rgb_t.element_size()
        assert rgb_t.dim() == 4 and rgb_t.shape[1] == 3 and rgb_t.shape[2] >= out_h and rgb_t.shape[3] >= out_w and rgb_t.stride(3) == 1
        row_stride, image_stride = rgb_row_stride or rgb_t.stride(2) * es, rgb_t.stride(0) * es
        if isinstance(fmt, OutputSpec):
            fmt.plane_stride = rgb_t.stride(1) * es
    else:
        if scale != 1 or q.roi is not None or q.target is not None:
            if q.roi is None and q.target is None:
                out_w, out_h = scaled_size(desc.width, desc.height, scale)
            assert rgb_t.shape[1] >= out_h and (rgb_row_stride or rgb_t.stride(1)) >= 3 * out_w, "rgb_t is smaller than the scaled images"
        row_stride, image_stride = rgb_row_stride or rgb_t.stride(1), rgb_t.stride(0)
    b = DeviceBatch()
    b.desc = desc
    b.n_images = n_images
    b.d_coef = coef_t.data_ptr()
    b.coef_image_stride = coef_t.stride(0) * 2 if n_images > 1 else coef_t.numel() * 2
    b.d_qtabs = qtabs_t.data_ptr()
    b.qtab_image_stride = 0 if shared_qtabs else 768
    b.d_rgb = rgb_t.data_ptr()
    b.rgb_row_stride = row_stride
    b.rgb_image_stride = image_stride
    return b
