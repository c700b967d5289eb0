"""jpeg_decoder_amd -- MI355X-native JPEG block pipeline (dequantize -> 8x8 IDCT -> YCbCr->RGB).

The product is the C-ABI shared library ``libjpegblk.so`` (include/jpegblk.h, sources under
``csrc/``: hand-written HIP kernels for gfx950 + the C++ host side).  This Python package is a
thin ctypes binding over that ABI, used by tests/, bench.py and __graft_entry__.py; PyTorch is
used only as plumbing (device memory, streams, torch.distributed).

There is no CPU fallback: if the library is missing, or no HIP device is usable, calls fail
loudly (ImportError / JbError).
"""
from .api import (JbError, Context, ImageDesc, Geometry, DeviceBatch, lib, lib_path, make_desc,
                  geometry_of, flat_front_geometry, resolve_qtabs, entropy_decode, decode_batch, BatchDecoder, build_library, scaled_size,
                  OutputSpec, output_bytes, torch_batch, FMT_RGB_U8_HWC, FMT_RGB_U8_CHW, FMT_RGB_F32_CHW, FMT_RGB_F16_CHW,
                  FMT_DTYPE, Roi, roi_check, resize_check, crops_check, Resize, filter_check, filter_window,
                  FILTER_AREA, FILTER_BILINEAR, FILTER_BICUBIC, ARITH_REFERENCE, ARITH_LIBJPEG,
                  ORIENT_EXIF, ORIENT_STORED, exif_orientation, oriented_size, orient_map_roi,
                  View, VIEW_MIRROR, VIEWS_MAX, views_check, ViewGroup, ViewOutput, VIEW_GROUPS_MAX, view_groups_check, view_groups_bytes,
                  Fit, FitGeometry, fit_geometry, FIT_STRETCH, FIT_PAD, FIT_COVER, FIT_CENTER, FIT_START, FIT_END,
                  DraftGeometry, draft_geometry,
                  ColorOp, ColorChain, color_check, color_host, COLOR_OPS_MAX, blur_params, COLOR_BLUR, COLOR_BLUR_BOX_MAX,
                  COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION, COLOR_HUE, COLOR_GRAYSCALE, COLOR_SOLARIZE,
                  COLOR_POSTERIZE, COLOR_INVERT, COLOR_AUTOCONTRAST, COLOR_EQUALIZE, COLOR_SHARPNESS, COLOR_STATS_MAX, color_lut,
                  COLOR_SHEAR_X, COLOR_SHEAR_Y, COLOR_TRANSLATE_X, COLOR_TRANSLATE_Y, COLOR_ROTATE, COLOR_WARPS_MAX, WARP_SHIFT, WARP_FIXED,
                  warp_params)
from .crops import random_resized_crop, random_views, random_multicrop
from .color import (color_jitter, random_apply, random_grayscale, random_solarize, dino_color, hue_shift, random_blur, dino_augment,
                    posterize, invert, autocontrast, equalize, sharpness, rand_augment_color, trivial_augment_wide_color,
                    shear_x, shear_y, translate_x, translate_y, rotate, rand_augment, trivial_augment_wide)

__all__ = ["JbError", "Context", "ImageDesc", "Geometry", "DeviceBatch", "lib", "lib_path",
           "make_desc", "geometry_of", "flat_front_geometry", "resolve_qtabs", "entropy_decode", "decode_batch", "BatchDecoder", "build_library",
           "scaled_size", "OutputSpec", "output_bytes", "torch_batch", "FMT_RGB_U8_HWC", "FMT_RGB_U8_CHW", "FMT_RGB_F32_CHW",
           "FMT_RGB_F16_CHW", "FMT_DTYPE", "Roi", "roi_check", "resize_check", "crops_check",
           "random_resized_crop", "Resize", "filter_check", "filter_window", "FILTER_AREA", "FILTER_BILINEAR", "FILTER_BICUBIC",
           "ARITH_REFERENCE", "ARITH_LIBJPEG", "ORIENT_EXIF", "ORIENT_STORED", "exif_orientation", "oriented_size",
           "orient_map_roi", "View", "VIEW_MIRROR", "VIEWS_MAX", "views_check", "random_views", "ViewGroup", "ViewOutput", "VIEW_GROUPS_MAX", "view_groups_check", "view_groups_bytes",
           "random_multicrop",
           "Fit", "FitGeometry", "fit_geometry", "FIT_STRETCH", "FIT_PAD", "FIT_COVER", "FIT_CENTER", "FIT_START", "FIT_END",
           "DraftGeometry", "draft_geometry",
           "ColorOp", "ColorChain", "color_check", "color_host", "COLOR_OPS_MAX", "COLOR_BRIGHTNESS", "COLOR_CONTRAST",
           "COLOR_SATURATION", "COLOR_HUE", "COLOR_GRAYSCALE", "COLOR_SOLARIZE",
           "color_jitter", "random_apply", "random_grayscale", "random_solarize", "dino_color", "hue_shift",
           "blur_params", "COLOR_BLUR", "COLOR_BLUR_BOX_MAX", "random_blur", "dino_augment",
           "COLOR_POSTERIZE", "COLOR_INVERT", "COLOR_AUTOCONTRAST", "COLOR_EQUALIZE", "COLOR_SHARPNESS", "COLOR_STATS_MAX", "color_lut",
           "posterize", "invert", "autocontrast", "equalize", "sharpness", "rand_augment_color", "trivial_augment_wide_color",
           "COLOR_SHEAR_X", "COLOR_SHEAR_Y", "COLOR_TRANSLATE_X", "COLOR_TRANSLATE_Y", "COLOR_ROTATE", "COLOR_WARPS_MAX", "WARP_SHIFT",
           "WARP_FIXED", "warp_params", "shear_x", "shear_y", "translate_x", "translate_y", "rotate", "rand_augment", "trivial_augment_wide"]
