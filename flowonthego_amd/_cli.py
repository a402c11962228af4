"""What the command-line modules (python -m flowonthego_amd.<tool>) do in the same way, written once: the counterpart of _args.py
for the tools.  Loading the input files and refusing the ones a tool cannot use with one line "<tool>: <message>" and return
value 1; the context of a frame sequence; the way onto the device; the PNGs the tools put out.  A tool keeps its text, its parser
and its argument errors, its own call of the feature and its print lines.  numpy and torch are imported at the call: a tool decides
its argument errors before either is loaded."""
import sys
import zlib

from ._png import read_gray_png, write_png

# the colours of a per-pixel code where 0 is the good case (white), 1 the exception (red), 2 masked (gray), 3 unknown (black)
CODE_RGB = ((255, 255, 255), (220, 30, 30), (128, 128, 128), (0, 0, 0))


class Refusal(Exception):
    """an input file the tool cannot use; the message names the file"""


class refusing:
    """with refusing("<tool>") as inputs: load and check the input files
       if inputs.refused: return 1
    A Refusal, and what the readers raise for a file that is missing or not of its kind, becomes the line "<tool>: <message>" on
    stderr.  Only the loading belongs inside: whatever the computation raises is the caller's to see."""

    def __init__(self, tool):
        self.tool, self.refused = tool, False

    def __enter__(self):
        return self

    def __exit__(self, kind, e, tb):
        if kind is None or not issubclass(kind, (Refusal, OSError, ValueError, zlib.error)):
            return False
        sys.stderr.write("%s: %s\n" % (self.tool, e))
        self.refused = True
        return True


# --- loaders: a path that is None (an option not given) loads as None, and every check below lets None pass

def load_flow(path):
    """a .flo file -> (h, w, 2) float32"""
    from .flo import read_flo
    return None if path is None else read_flo(path)


def load_array(path):
    """an .npy file -> the array"""
    import numpy as np
    return None if path is None else np.load(path)


def load_mask_png(path):
    """an 8-bit gray PNG -> (h, w) uint8"""
    return None if path is None else read_gray_png(path)


# --- checks: one wording per kind of refusal

def _size(shape):
    return " x ".join("%d" % v for v in tuple(shape[:2])[::-1]) if len(shape) >= 2 else "of shape %s" % (tuple(shape),)


def mask_like_flow(mask, path, h, w, dtype="uint8"):
    """a value per pixel (a mask PNG, an array of codes or of ids) has the flow's size and the type it needs"""
    if mask is not None and (mask.shape != (h, w) or str(mask.dtype) != dtype):
        raise Refusal("%s is %s %s, the flow takes %s %d x %d" % (path, mask.dtype, _size(mask.shape), dtype, w, h))
    return mask


def flow_like_flow(other, other_path, flow, path):
    """a second flow (the backward flow, the next flow of a sequence) has the first one's size"""
    if other is not None and other.shape != flow.shape:
        raise Refusal("%s is %s, %s is %s" % (path, _size(flow.shape), other_path, _size(other.shape)))
    return other


def frame_like_flow(frame, path, h, w, dtypes=("uint8", "float32")):
    """a frame or guide is (h, w), (h, w, 1) or (h, w, 3) of the flow's size and of one of the types"""
    if frame is not None and (str(frame.dtype) not in dtypes or frame.shape not in ((h, w), (h, w, 1), (h, w, 3))):
        raise Refusal("%s must hold an (%d, %d) or (%d, %d, 3) %s array (the flow's size)" % (path, h, w, h, w, " or ".join(dtypes)))
    return frame


def array_like_array(x, path, first, first_path):
    """a second frame, or the reference to compare with, has the shape and type of the first"""
    if x is not None and (x.shape != first.shape or x.dtype != first.dtype):
        raise Refusal("%s must have the shape and type of %s" % (path, first_path))
    return x


def frame_sequence(path, min_frames, label, c1):
    """frames.npy -> its (label, h, w) or (label, h, w, 3) uint8 or float32 array of at least min_frames frames, as loaded; c1: a
    trailing channel of 1 is taken as well, for drop_c1() to remove"""
    frames = load_array(path)
    if frames.ndim not in (3, 4) or frames.shape[0] < min_frames or str(frames.dtype) not in ("uint8", "float32") \
            or (frames.ndim == 4 and frames.shape[3] not in ((1, 3) if c1 else (3,))):
        raise Refusal("%s must hold a (%s, h, w) or (%s, h, w, 3) uint8 or float32 array of at least %d frame%s"
                      % (path, label, label, min_frames, "s" if min_frames > 1 else ""))
    return frames


def drop_c1(frames):
    """(T, h, w, 1) -> (T, h, w)"""
    return frames[..., 0] if frames is not None and frames.ndim == 4 and frames.shape[3] == 1 else frames


# --- the device

def sequence_context(frames, op_point, bidir, max_batch):
    """the OFClass for the flows of frames (T, h, w) or (T, h, w, 3) at an operating point: gray frames on one channel; 8-bit colour
    frames on one channel as well, made gray from R, G, B on load; float32 colour frames on three channels"""
    from . import img_params, operating_point
    from .oflow import OFClass
    h, w = frames.shape[1:3]
    u8_rgb = frames.ndim == 4 and str(frames.dtype) == "uint8"
    op = operating_point(op_point, w, 3 if frames.ndim == 4 and not u8_rgb else 1)
    op.bidir = bool(bidir)
    if u8_rgb:
        op.u8_color = 2
    return OFClass(op, img_params(width=w, height=h), max_batch=max_batch)


def to_device(x):
    """a host array -> a tensor on the current device"""
    import numpy as np
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def occlusion_mask(flow, bw):
    """--bw: the forward-backward check of the two flows on the device, its mask keeps inconsistent vectors out of the feature"""
    from .consistency import fb_check
    return None if bw is None else fb_check(flow, bw)[0]


# --- output

def save_frame_png(path, img, h, w):
    """a gray or colour frame, uint8 or float32 (rounded and clipped to 0 .. 255, not-a-number to 0), tensor or array -> an RGB PNG"""
    import numpy as np
    if hasattr(img, "detach"):
        img = img.detach().cpu().numpy()
    img = img.reshape(h, w, -1)
    if img.dtype != np.uint8:
        img = np.clip(np.rint(np.nan_to_num(img)), 0, 255).astype(np.uint8)
    write_png(path, np.ascontiguousarray(np.broadcast_to(img, (h, w, 3))))


def save_code_png(path, code, palette=CODE_RGB):
    """a per-pixel code (h, w), tensor or array -> the PNG of palette[code]"""
    import numpy as np
    if hasattr(code, "detach"):
        code = code.detach().cpu().numpy()
    write_png(path, np.asarray(palette, np.uint8)[code])
