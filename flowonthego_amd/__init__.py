"""flowonthego_amd -- MI355X-native Dense-Inverse-Search optical flow.

Host-side mirror of the reference's flow API (src/oflow.h, src/patchgrid.h, src/refine_variational.h, src/params.h)
over the C-ABI of libfotg.so (include/fotg.h), whose kernels are hand-written HIP for gfx950.
"""
from ._lib import FotgError, LIB_PATH, lib  # noqa: F401
from .params import AutoFirstScaleSelect, img_params, opt_params, operating_point, padded_size  # noqa: F401


def _names(module, *names):
    return {n: (module, n) for n in names}


# the lazy names of the package: name -> (module, attribute).  The torch-dependent modules are imported at the first use of one of
# their names, so the CPU-only checks (symbol export, host logic) stay light.  An add-on adds its line here.
LAZY = {
    **_names("oflow", "OFClass", "PatGridClass", "VarRefClass", "gradient_magnitude"),
    **_names("color", "flow_to_color", "color_wheel"),
    **_names("_png", "write_png"),
    **_names("consistency", "fb_check", "upsample_crop_fb_check"),
    **_names("warp", "warp", "upsample_crop_warp"),
    **_names("temporal", "temporal_filter", "upsample_crop_temporal_filter"),
    **_names("flowfilter", "upsample_crop_filter_flow", "spatial_table"),
    **_names("blockmotion", "upsample_crop_block_motion"),
    **_names("chain", "chain", "track_points", "upsample_crop_chain", "upsample_crop_track_points"),
    **_names("motion", "motion_flow", "upsample_crop_fit_motion", "smoothing_motions", "MODELS", "CODES"),
    **_names("objects", "label_components", "object_summary", "OBJECT", "OBJECT_STATS"),
    **_names("tracks", "object_overlap", "upsample_crop_object_overlap", "object_links", "link_tracks", "TRACK", "TRACK_STATS"),
    **_names("histograms", "upsample_crop_motion_histograms", "motion_descriptors", "HIST"),
    **_names("motionblur", "upsample_crop_motion_blur"),
    "BLUR_STATS": ("motionblur", "STATS"),
    **_names("plate", "background_plate", "upsample_crop_background_plate", "plate_motions", "mosaic_canvas"),
    **_names("layers", "upsample_crop_motion_layers", "layer_summary", "LAYER", "LAYER_STATS", "UNASSIGNED", "MASKED", "UNKNOWN"),
    **_names("subtract", "subtract_background", "upsample_crop_subtract_background", "frame_motions", "foreground_objects", "foreground_mask"),
    **_names("erase", "upsample_crop_remove_objects", "grow_mask"),    # (remove_objects: the callable tool module below)
    **_names("morph", "morphology"),                                   # (clean_mask: the callable tool module below)
    **_names("fill", "fill_flow", "fill_removed", "upsample_crop_fill_flow", "FILL_CODES", "FILL_STATS"),      # (fill_holes: the callable tool module below)
    **_names("interp", "interpolate", "upsample_crop_interpolate"),
    **_names("pipeline", "FlowPipeline"),
    **_names("node", "FlowNode"),
}

# the command-line modules that are returned as modules: each is callable as the function of its name in flowonthego_amd.flowfilter /
# blockmotion / motion / objects / tracks / histograms / motionblur / plate / layers / subtract / erase / morph / fill
CLI_MODULES = ["filter_flow", "block_motion", "fit_motion", "stabilize", "moving_objects", "track_objects", "motion_histograms", "motion_blur", "background", "motion_layers", "foreground", "remove_objects", "clean_mask", "fill_holes"]


def __getattr__(name):
    import importlib
    if name in CLI_MODULES:
        return importlib.import_module("." + name, __name__)
    if name in LAZY:
        module, attr = LAZY[name]
        return getattr(importlib.import_module("." + module, __name__), attr)
    raise AttributeError(name)
