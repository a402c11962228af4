"""Host-side tests of the connected-component labelling (no GPU needed): the numpy restatement (tests/objects_ref.py) against
hand-written 5 x 5 cases whose labels and records are spelled out here, its invariants on seeded random maps, the selection by
min_area and max_objects, the argument contract of fotg_label_components through ctypes (every refused combination returns
FOTG_ERR_ARG before the device is touched: the pointers given are null or host memory), and the new header and example compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import objects_ref as R
from conftest import ROOT
from host_checks import run_cli

FOTG_ERR_ARG = 1

# two blobs that touch only diagonally ((1,1) - (2,2)), and a single pixel that touches nothing
A = np.array([[1, 1, 0, 0, 0],
              [1, 1, 0, 0, 0],
              [0, 0, 1, 1, 0],
              [0, 0, 1, 0, 0],
              [0, 0, 0, 0, 1]], np.uint8)
# a U whose arms join only in row 3 (the right arm's first label 3 must give way to 1), code-2 pixels touching it diagonally / below
B = np.array([[0, 1, 0, 1, 0],
              [0, 1, 0, 1, 0],
              [0, 1, 0, 1, 0],
              [0, 1, 1, 1, 0],
              [2, 0, 0, 0, 2]], np.uint8)


def rows(*recs, max_objects=4):
    out = np.zeros((max_objects, 11), np.int64)
    for i, r in enumerate(recs):
        out[i, :len(r)] = r
    return out


def test_hand_case_diagonal_blobs():
    r8 = R.components(A, R.fg_set((1,)), 8, max_objects=4)
    assert np.array_equal(r8["labels"], np.array([[0, 0, -1, -1, -1],
                                                  [0, 0, -1, -1, -1],
                                                  [-1, -1, 0, 0, -1],
                                                  [-1, -1, 0, -1, -1],
                                                  [-1, -1, -1, -1, 24]], np.int32))
    #                                      label area box          sum x, sum y
    assert np.array_equal(r8["objects"], rows([0, 7, 0, 0, 3, 3, 9, 9], [24, 1, 4, 4, 4, 4, 4, 4]))
    assert np.array_equal(r8["ids"], np.where(r8["labels"] == 0, 0, np.where(r8["labels"] == 24, 1, -1)))
    assert r8["stats"].tolist() == [8, 2, 2, 2]
    r4 = R.components(A, R.fg_set((1,)), 4, max_objects=4)
    assert np.array_equal(r4["labels"], np.array([[0, 0, -1, -1, -1],
                                                  [0, 0, -1, -1, -1],
                                                  [-1, -1, 12, 12, -1],
                                                  [-1, -1, 12, -1, -1],
                                                  [-1, -1, -1, -1, 24]], np.int32))
    assert np.array_equal(r4["objects"], rows([0, 4, 0, 0, 1, 1, 2, 2], [12, 3, 2, 2, 3, 3, 7, 7], [24, 1, 4, 4, 4, 4, 4, 4]))
    assert r4["stats"].tolist() == [8, 3, 3, 3]
    assert r8["labels"].dtype == np.int32 and r8["ids"].dtype == np.int32 and r8["objects"].dtype == np.int64


def test_hand_case_u_shape_codes_and_values():
    lab1 = np.where(B == 1, 1, -1).astype(np.int32)
    for conn in (4, 8):
        r = R.components(B, R.fg_set((1,)), conn, max_objects=4)
        assert np.array_equal(r["labels"], lab1)
        assert np.array_equal(r["objects"], rows([1, 9, 1, 0, 3, 3, 18, 15]))
        assert r["stats"].tolist() == [9, 1, 1, 1]
    # code 2 is foreground as well: at 8 the two corner pixels hang on the U diagonally, at 4 they stand alone
    r = R.components(B, R.fg_set((1, 2)), 8, max_objects=4)
    assert np.array_equal(r["labels"], np.where(B > 0, 1, -1))
    assert np.array_equal(r["objects"], rows([1, 11, 0, 0, 4, 4, 22, 23]))
    r = R.components(B, R.fg_set((1, 2)), 4, max_objects=4)
    lab = lab1.copy()
    lab[4, 0], lab[4, 4] = 20, 24
    assert np.array_equal(r["labels"], lab)
    assert np.array_equal(r["objects"], rows([1, 9, 1, 0, 3, 3, 18, 15], [20, 1, 0, 4, 0, 4, 0, 4], [24, 1, 4, 4, 4, 4, 4, 4]))
    # only code 2: codes >= 8 are never foreground, whatever the set
    C8 = B.copy()
    C8[0, 0] = 9
    assert R.components(C8, 255, 4, max_objects=4)["labels"][0, 0] == -1
    # values: u = x, v = -y / 2; a NaN at (x 1, y 0), 5000 px at (x 3, y 0), an infinity on a background pixel
    val = np.zeros((5, 5, 2), np.float32)
    val[..., 0] = np.arange(5)[None, :]
    val[..., 1] = -0.5 * np.arange(5)[:, None]
    val[0, 1, 0] = np.nan
    val[0, 3, 1] = 5000.0
    val[0, 0, 0] = np.inf
    r = R.components(B, R.fg_set((1,)), 8, values=val, max_objects=4)
    assert np.array_equal(r["objects"], rows([1, 9, 1, 0, 3, 3, 18, 15, 7, 256 * 14, -128 * 15]))
    assert np.array_equal(R.summary(r["objects"])[0], [2.0, 15 / 9, 2.0, -15 / 14])
    assert np.isnan(R.summary(r["objects"])[1]).all()


@pytest.mark.parametrize("conn", [4, 8])
def test_label_is_the_minimum_linear_index(conn):
    rng = np.random.default_rng(conn)
    for w, h, d in ((31, 17, 0.3), (23, 29, 0.6), (40, 9, 0.9), (1, 7, 0.6), (9, 1, 0.6)):
        code = (rng.random((h, w)) < d).astype(np.uint8)
        r = R.components(code, 2, conn, max_objects=h * w)
        lab = r["labels"]
        assert np.array_equal(lab >= 0, code == 1)
        lin = np.arange(h * w).reshape(h, w)
        for l in np.unique(lab[lab >= 0]):
            assert lin[lab == l].min() == l
        # neighbours share a label, and (by an independent flood fill) nothing else does
        same = lambda a, b: np.all(a[(a >= 0) & (b >= 0)] == b[(a >= 0) & (b >= 0)])
        assert same(lab[:, 1:], lab[:, :-1]) and same(lab[1:], lab[:-1])
        if conn == 8:
            assert same(lab[1:, 1:], lab[:-1, :-1]) and same(lab[1:, :-1], lab[:-1, 1:])
        seen = np.zeros((h, w), bool)
        for l in np.unique(lab[lab >= 0]):
            stack, n = [divmod(int(l), w)], 0
            seen[stack[0]] = True
            while stack:
                y, x = stack.pop()
                n += 1
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if (dy or dx) and (conn == 8 or not (dy and dx)):
                            yy, xx = y + dy, x + dx
                            if 0 <= yy < h and 0 <= xx < w and code[yy, xx] == 1 and not seen[yy, xx]:
                                seen[yy, xx] = True
                                stack.append((yy, xx))
            assert n == (lab == l).sum() == r["objects"][r["objects"][:, 0] == l][0, 1]
        assert np.array_equal(seen, code == 1)
        assert r["stats"][1] == len(np.unique(lab[lab >= 0]))


def test_min_area_and_max_objects_select_what_the_definition_says():
    rng = np.random.default_rng(7)
    code = (rng.random((24, 37)) < 0.45).astype(np.uint8)
    full = R.components(code, 2, 4, max_objects=1000)
    nall = int(full["stats"][1])
    allrows = full["objects"][:nall]
    assert nall > 20 and np.all(np.diff(allrows[:, 0]) > 0) and not full["objects"][nall:].any()
    big = allrows[allrows[:, 1] >= 3]
    assert 5 < len(big) < nall
    r = R.components(code, 2, 4, min_area=3, max_objects=5)
    assert np.array_equal(r["objects"], big[:5])
    assert r["stats"].tolist() == [int((code == 1).sum()), nall, len(big), 5]
    assert np.array_equal(r["labels"], full["labels"])                      # small components keep their label
    for row in range(5):
        assert np.array_equal(r["ids"] == row, full["labels"] == big[row, 0])
    assert set(np.unique(r["ids"])) == {-1, 0, 1, 2, 3, 4}
    r = R.components(code, 2, 4, min_area=3, max_objects=len(big) + 3)
    assert np.array_equal(r["objects"][:len(big)], big) and not r["objects"][len(big):].any()
    assert r["stats"].tolist()[2:] == [len(big), len(big)]
    none = R.components(code, 2, 4, min_area=10 ** 6, max_objects=3)
    assert not none["objects"].any() and (none["ids"] == -1).all() and none["stats"].tolist()[2:] == [0, 0]


def test_refused_arguments_return_err_arg_before_the_device_is_touched():
    import flowonthego_amd as F
    L = F.lib()
    host = C.create_string_buffer(64)                   # never read: every call below is refused before anything is launched
    ptr = C.cast(host, C.c_void_p)
    good = dict(device=0, n=1, code=ptr, w=8, h=8, fg=2, conn=8, values=None, min_area=1, max_objects=4, labels=None, ids=None,
                objects=ptr, stats=None)
    bad = [dict(fg=0), dict(fg=256), dict(conn=6), dict(min_area=0), dict(max_objects=0), dict(max_objects=65537), dict(w=0),
           dict(w=16385), dict(h=0), dict(h=16385), dict(n=0), dict(code=None), dict(objects=None)]
    for change in bad:
        for null_all in (False, True):
            a = dict(good, **change)
            if null_all:
                a.update(code=None, objects=None)
            st = L.fotg_label_components(a["device"], a["n"], a["code"], a["w"], a["h"], a["fg"], a["conn"], a["values"], a["min_area"],
                                         a["max_objects"], a["labels"], a["ids"], a["objects"], a["stats"], None)
            assert st == FOTG_ERR_ARG, (change, null_all)
    tw, th = C.c_int(0), C.c_int(0)
    assert L.fotg_components_tile(C.byref(tw), C.byref(th)) == 0 and L.fotg_components_tile(None, None) == 0
    assert tw.value >= 1 and th.value >= 1
    import flowonthego_amd.objects as O
    assert O.TILE == (tw.value, th.value)


def test_entry_points_are_declared_bound_and_documented():
    import flowonthego_amd as F
    from flowonthego_amd._lib import SYMBOLS
    L = F.lib()
    hdr = open(os.path.join(ROOT, "include", "fotg.h")).read()
    bound = {s[0]: s for s in SYMBOLS}
    for name in ("fotg_label_components", "fotg_components_tile"):
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert name in bound and hasattr(L, name) and len(decl.split(",")) == len(bound[name][2]), name
    assert "fotg_label_components(" in open(os.path.join(ROOT, "include", "fotg", "objects.h")).read()
    for name in ("label_components", "moving_objects", "object_summary"):
        assert callable(getattr(F, name)), name
    assert F.OBJECT == R.OBJECT and F.OBJECT_STATS == R.OBJECT_STATS and len(F.OBJECT) == 11
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.moving_objects)
    # the definition and why no sum overflows, at the head of the kernels and in the public header
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "components.hip.h")).read()
    for text in (head, hdr):
        assert "2^48" in text and "2^42" in text and "16384" in text and "minimum linear index" in text


def test_moving_objects_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "moving_objects")
    assert os.path.exists(exe)
    for args in ([], ["a.flo", "0"], ["a.flo", "5", "x"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_cli_argument_errors():
    for args in ([], ["a.flo", "b.flo"], ["a.flo", "--connectivity", "6"], ["a.flo", "--min-area", "0"], ["a.flo", "--max-objects", "70000"],
                 ["a.flo", "--model", "projective"], ["a.flo", "--ids"]):
        r = run_cli("moving_objects", args)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_component_kernels_without_scratch():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "flowonthego_amd", "csrc")], stdout=subprocess.DEVNULL)
    txt = open(os.path.join(ROOT, "flowonthego_amd", "libfotg.resusage.txt")).read()
    names = re.findall(r"Function Name: (\S+)", txt)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(names) == len(scratch)
    table = dict(zip(names, scratch))
    want = ["comp_tile_kernelE", "comp_merge_kernelE", "comp_flatten_kernelE", "comp_count_kernelE", "comp_scan_kernelE", "comp_emit_kernelE",
            "comp_reduce_kernelILb0E", "comp_reduce_kernelILb1E"]
    for k in want:
        hit = [n for n in names if k in n]
        assert len(hit) == 1 and table[hit[0]] == 0, k
    assert len([n for n in names if "4fotg" in n and "comp_" in n]) == len(want)
