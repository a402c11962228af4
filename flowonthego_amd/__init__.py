"""flowonthego_amd -- MI355X-native Dense-Inverse-Search optical flow.

Host-side mirror of the reference's flow API (src/oflow.h, src/patchgrid.h, src/refine_variational.h, src/params.h)
over the C-ABI of libfotg.so (include/fotg.h), whose kernels are hand-written HIP for gfx950.
"""
from ._lib import FotgError, LIB_PATH, lib  # noqa: F401
from .params import AutoFirstScaleSelect, img_params, opt_params, operating_point, padded_size  # noqa: F401


def __getattr__(name):
    # torch-dependent classes are imported lazily so the CPU-only checks (symbol export, host logic) stay light
    if name in ("OFClass", "PatGridClass", "VarRefClass", "gradient_magnitude"):
        from . import oflow
        return getattr(oflow, name)
    if name in ("flow_to_color", "write_png", "color_wheel"):
        from . import color
        return getattr(color, name)
    if name in ("fb_check", "upsample_crop_fb_check"):
        from . import consistency
        return getattr(consistency, name)
    if name in ("warp", "upsample_crop_warp"):
        import importlib
        return getattr(importlib.import_module(".warp", __name__), name)
    if name in ("temporal_filter", "upsample_crop_temporal_filter"):
        import importlib
        return getattr(importlib.import_module(".temporal", __name__), name)
    if name in ("upsample_crop_filter_flow", "spatial_table"):
        from . import flowfilter
        return getattr(flowfilter, name)
    if name == "filter_flow":
        # (the command-line module of this name; it is callable as flowonthego_amd.flowfilter.filter_flow)
        import importlib
        return importlib.import_module(".filter_flow", __name__)
    if name == "upsample_crop_block_motion":
        from . import blockmotion
        return blockmotion.upsample_crop_block_motion
    if name == "block_motion":
        # (the command-line module of this name; it is callable as flowonthego_amd.blockmotion.block_motion)
        import importlib
        return importlib.import_module(".block_motion", __name__)
    if name in ("chain", "track_points", "upsample_crop_chain", "upsample_crop_track_points"):
        import importlib
        return getattr(importlib.import_module(".chain", __name__), name)
    if name in ("motion_flow", "upsample_crop_fit_motion", "smoothing_motions", "MODELS", "CODES"):
        from . import motion
        return getattr(motion, name)
    if name in ("label_components", "object_summary", "OBJECT", "OBJECT_STATS"):
        from . import objects
        return getattr(objects, name)
    if name in ("object_overlap", "upsample_crop_object_overlap", "object_links", "link_tracks", "TRACK", "TRACK_STATS"):
        from . import tracks
        return getattr(tracks, name)
    if name in ("upsample_crop_motion_histograms", "motion_descriptors", "HIST"):
        from . import histograms
        return getattr(histograms, name)
    if name in ("upsample_crop_motion_blur", "BLUR_STATS"):
        from . import motionblur
        return getattr(motionblur, "STATS" if name == "BLUR_STATS" else name)
    if name in ("fit_motion", "stabilize", "moving_objects", "track_objects", "motion_histograms", "motion_blur"):
        # (the command-line modules of these names; each is callable as the function of flowonthego_amd.motion / objects / tracks /
        # histograms / motionblur)
        import importlib
        return importlib.import_module("." + name, __name__)
    if name in ("interpolate", "upsample_crop_interpolate"):
        from . import interp
        return getattr(interp, name)
    if name == "FlowPipeline":
        from .pipeline import FlowPipeline
        return FlowPipeline
    if name == "FlowNode":
        from .node import FlowNode
        return FlowNode
    raise AttributeError(name)
