"""What the host-side test files (test_host_*.py) of the add-ons check in the same way, written once: the entry points of a feature
through the header, the bindings, the library and the C++ shim; the compiler's resource table; the refusals of a command-line tool.
No GPU needed."""
import os
import re
import struct
import subprocess
import sys
import zlib

from conftest import ROOT


def entry_points(symbols, shim_header, in_shim=None):
    """every symbol is declared in include/fotg.h, bound in _lib.SYMBOLS with one ctypes argument per declared parameter, exported by
    the library, and (those of in_shim, by default all) called by include/fotg/<shim_header>: (the package, the header's text)"""
    import flowonthego_amd as F
    from flowonthego_amd._lib import SYMBOLS
    L = F.lib()
    hdr = open(os.path.join(ROOT, "include", "fotg.h")).read()
    bound = {s[0]: s for s in SYMBOLS}
    for name in symbols:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound and hasattr(L, name)
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(bound[name][2]), name
    shim = open(os.path.join(ROOT, "include", "fotg", shim_header)).read()
    for name in (symbols if in_shim is None else in_shim):
        assert name + "(" in shim
    return F, hdr


def resource_table():
    """the kernels of the built library by the compiler's resource remarks: (names, table) -- the mangled names as listed (a kernel
    compiled in two files is listed twice) and name -> private-memory bytes per lane"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "flowonthego_amd", "csrc")], stdout=subprocess.DEVNULL)
    txt = open(os.path.join(ROOT, "flowonthego_amd", "libfotg.resusage.txt")).read()
    names = re.findall(r"Function Name: (\S+)", txt)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(names) == len(scratch)
    return names, dict(zip(names, scratch))


def run_cli(module, args):
    """python -m flowonthego_amd.<module> with the arguments, in a child process on this tree: the finished process, its output as text"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "flowonthego_amd." + module] + list(args), capture_output=True, text=True, cwd=ROOT, env=env)


def cli_refuses(module, arg_lists):
    """python -m flowonthego_amd.<module> with each of the argument lists ends with an error and its usage line"""
    for args in arg_lists:
        r = run_cli(module, args)
        assert r.returncode != 0 and "usage" in r.stderr, (module, args)


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def gray_png_bytes(img, rows=None):
    """an (h, w) uint8 array as an 8-bit gray PNG with row filter 0; rows: how many of its rows the data stream holds (default all)"""
    h, w = img.shape
    raw = b"".join(b"\0" + img[y].tobytes() for y in range(h if rows is None else rows))
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + _png_chunk(b"IDAT", zlib.compress(raw))
            + _png_chunk(b"IEND", b""))


def read_png_rgb(path):
    """the single-IDAT, filter-0 RGB PNGs write_png writes"""
    import numpy as np
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", None, None
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)
