"""The PNG codec of the package (zlib + struct only): the writer of the 8-bit RGB images the tools put out and the reader of the
8-bit gray masks they take.  Host-side only; numpy is imported at the call, so that a command-line module may import this one
before it has looked at its arguments."""
import struct
import zlib


def write_png(path, rgb):
    """rgb: (h, w, 3) uint8 (numpy or tensor) -> an 8-bit RGB PNG (zlib + struct only)"""
    import numpy as np
    if hasattr(rgb, "detach"):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("rgb must be a non-empty (h, w, 3) uint8 array, got %s %s" % (rgb.dtype, rgb.shape))
    h, w = rgb.shape[:2]

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    raw = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], axis=1).tobytes()   # filter type 0 per row
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(chunk(b"IEND", b""))


def read_gray_png(path):
    """an 8-bit gray, non-interlaced PNG -> (h, w) uint8 (zlib + struct only)"""
    import numpy as np
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s is not a PNG file" % path)
    pos, idat, head = 8, b"", None
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            break
    if head is None or head[2:] != (8, 0, 0, 0, 0):
        raise ValueError("%s must be an 8-bit gray PNG without interlacing" % path)
    w, h = head[:2]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8)
    if raw.size != h * (w + 1):
        raise ValueError("%s is truncated" % path)
    rows = raw.reshape(h, w + 1)
    out = np.zeros((h, w), np.uint8)
    prev = np.zeros(w, np.int32)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):                   # the filters that look to the left: byte by byte
            cur = np.zeros(w, np.int32)
            for x in range(w):
                a, b, c = (cur[x - 1] if x else 0), prev[x], (prev[x - 1] if x else 0)
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (line[x] + p) & 255
        else:
            raise ValueError("%s: bad filter type %d" % (path, ft))
        out[y] = cur
        prev = cur
    return out
