"""The reference's own drivers, compiled UNCHANGED against the drop-in C++
API (gpu-accelerated-speech-recognition_amd/api over libasr_amd.so).

CPU: `make dropin` builds the reference's {main,nn_test}.cpp (skipped where
the reference checkout is absent).
GPU: tests/helpers/api_driver, this repository's own program over the same
classes (built by build()), is fed the drivers' inputs from tests/golden and
its results are checked against the reference's expected values (nn_test.cpp's
4 d.p. vectors; the main.cpp CTC vector's result under the CPU decoder's
semantics), so the GPU tests need no reference checkout.
"""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

REF = Path("/root/reference")
BIN = PKG / "build" / "dropin"


@pytest.mark.skipif(not (REF / "main.cpp").exists(), reason="reference checkout not present")
def test_reference_drivers_compile_unchanged():
    r = subprocess.run(["make", "-s", "-C", str(PKG), "dropin"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (BIN / "main").exists() and (BIN / "nn_test").exists()


DRIVER = ROOT / "tests" / "helpers" / "api_driver"


def _driver(args, numbers):
    """tests/helpers/api_driver (this repository's own program over api/,
    built by build()) with `numbers` on its stdin; returns its stdout."""
    assert DRIVER.exists(), "tests/helpers/api_driver missing: run build()"
    r = subprocess.run([str(DRIVER)] + [str(a) for a in args], input=" ".join(repr(float(x)) for x in numbers),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    return r.stdout


def _matrix(text, rows, cols):
    m = np.array([[float(x) for x in line.split()] for line in text.strip().splitlines()])
    assert m.shape == (rows, cols)
    return m


@pytest.mark.gpu
def test_nn_test_binary_matches_reference_kat():
    """The reference's Linear and RNN known-answer vectors (nn_test.cpp's
    inputs and its 4 d.p. expected values, tests/golden/nn_test_kat.json)
    through the C++ classes in a stand-alone program."""
    kat = json.loads((GOLDEN / "nn_test_kat.json").read_text())
    k = kat["linear"]
    lin = _matrix(_driver(["linear", k["M"], k["K"], k["N"]], k["input"] + k["weight"] + k["bias"]), k["M"], k["N"])
    assert np.abs(lin.flatten() - np.array(k["expected_4dp"])).max() < 1e-4
    k = kat["rnn"]
    rnn = _matrix(_driver(["rnn", k["T"], k["B"], k["in"], k["H"]],
                          k["input"] + k["w_ih"] + k["w_hh"] + k["b_ih"] + k["b_hh"]), k["T"] * k["B"], k["H"])
    assert np.abs(rnn.flatten() - np.array(k["expected_4dp"])).max() < 1e-4


@pytest.mark.gpu
def test_main_binary_ctc_result():
    """main.cpp's flow through the C++ classes in a stand-alone program: a
    randomly initialised Linear x3 -> RNN -> Linear x2 model, then its CTC
    vector (tests/golden/main_cpp_ctc.json) decoded by CTCBeamSearch; the
    result under the CPU decoder's semantics."""
    g = json.loads((GOLDEN / "main_cpp_ctc.json").read_text())
    out = _driver(["ctc", g["vocab"], g["T"], g["B"], g["beam"], g["blank"]], g["emissions"])
    best = [l.split() for l in out.splitlines() if l.startswith("best ")]
    assert len(best) == g["B"] == 1
    assert best[0][1] == "cbacbc"
    assert f"{float(best[0][2]):.6g}" == "0.00340885"
