"""What the host-side test files (test_host_*.py) of the add-ons check in the same way, written once: the entry points of a feature
through the header, the bindings, the library and the C++ shim; the compiler's resource table; the refusals of a command-line tool.
No GPU needed."""
import os
import re
import subprocess
import sys

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


def cli_refuses(module, arg_lists):
    """python -m flowonthego_amd.<module> with each of the argument lists ends with an error and its usage line"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for args in arg_lists:
        r = subprocess.run([sys.executable, "-m", "flowonthego_amd." + module] + list(args), capture_output=True, text=True, cwd=ROOT, env=env)
        assert r.returncode != 0 and "usage" in r.stderr, (module, args)
