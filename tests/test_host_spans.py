"""The aliasing rule of the add-on entry points (flowonthego_amd/csrc/spans.h), on the CPU: the header is plain C++, so it is
built with g++ -- with the address and undefined-behaviour sanitizers -- into a stand-alone driver (tests/spans_drv.cpp) that
compares overlap(), overlap_any() and overlap_among() with the rule restated there and exits non-zero on any mismatch.  No GPU:
what each entry point does with the answer is covered by the aliasing refusals of the tests/test_gpu_*.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_spans_follow_the_rule(tmp_path):
    exe = str(tmp_path / "spans_drv")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "spans_drv.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
