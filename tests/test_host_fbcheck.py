"""The consistency check's tools: examples/fb_check.cpp compiles and links against the C++ shim (no GPU needed), and the
python -m flowonthego_amd.fb_check CLI writes the mask PNG of the numpy restatement (GPU)."""
import os

import numpy as np
import pytest

import fbcheck_ref as R
from host_checks import cli_refuses, read_png_rgb, run_cli


def test_fb_check_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    assert os.path.exists(_build_example(tmp_path, "fb_check"))


def test_cli_argument_errors(tmp_path):
    cli_refuses("fb_check", ([], ["a.flo"], ["a.flo", "b.flo"], ["a.flo", "b.flo", "c.png", "--alpha1", "x"]))


@pytest.mark.gpu
def test_cli_writes_the_mask_of_the_restatement(tmp_path):
    from flowonthego_amd.flo import write_flo
    rng = np.random.default_rng(9)
    h, w = 23, 41
    fw = (rng.standard_normal((h, w, 2)) * 3).astype(np.float32)
    bw = (-fw + rng.standard_normal((h, w, 2)).astype(np.float32) * 0.4).astype(np.float32)
    fw[0, 0] = (np.nan, 0)
    a, b, out = (str(tmp_path / n) for n in ("fw.flo", "bw.flo", "mask.png"))
    write_flo(a, fw)
    write_flo(b, bw)
    r = run_cli("fb_check", [a, b, out, "--alpha1", "0.02", "--alpha2", "0.4"])
    assert r.returncode == 0, r.stderr
    want = R.fb_code(fw, bw, 0.02, 0.4)
    palette = np.array([(255, 255, 255), (255, 0, 0), (0, 0, 255), (0, 0, 0)], np.uint8)
    assert np.array_equal(read_png_rgb(out), palette[want])
    fr = [float(t) for t in r.stdout.split()[1::2]]
    assert np.allclose(fr, np.bincount(want.ravel(), minlength=4) / want.size, atol=1e-4)
