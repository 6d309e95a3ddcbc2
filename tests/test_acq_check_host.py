"""CPU test of the acquisition entry points' checks on their outputs and leading dimensions (csrc/agp_acq_check.h): the messages are
assembled from the words that differ between the entry points, so the COMPILED checks -- built for the host into
tests/c_host/acq_check_messages.cpp, a program of its own -- must say, byte for byte, what each entry point said when it carried its
own literal.  The literals below are those; the GPU suite and the users of the Python mirror read them.  Also here: which of
several faults is named, and what is not a fault (an unused leading dimension, an empty call).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgaussianprocesses.jl_amd", "csrc")
OK, INVALID = 0, 1  # AGP_OK, AGP_ERR_INVALID

EVAL = "n_t >= 0, xt and alpha_out must not be NULL, ldx >= D, ldg >= D when grad_out is given"
EVAL_JOINT = "n_sets >= 0, xq and alpha_out must not be NULL, ldx >= D, ldg >= D when grad_out is given"
NO_OUT, STARTS, LDX0 = "at least one output must be given", "n_starts >= 1 and below 2^31", "ldx0 >= D"
LDXO = "ldxo >= D when x_out is given"
STARTS_JOINT, LDB = "n_starts >= 1 and n_starts * 16 below 2^31", "ldb >= D when best_x is given"
A, P, J = "agp_svgp_acquisition: ", "agp_svgp_acquisition_pending: ", "agp_svgp_acquisition_joint: "
M, B, MJ = "agp_svgp_acq_maximize: ", "agp_svgp_acq_maximize_batch: ", "agp_svgp_acq_maximize_joint: "

WANT = [
    ("eval ok", OK, ""),
    ("eval empty", OK, ""),
    ("eval no grad, ldg unused", OK, ""),
    ("eval n < 0", INVALID, A + EVAL),
    ("eval xt NULL", INVALID, A + EVAL),
    ("eval alpha NULL", INVALID, A + EVAL),
    ("eval ldx", INVALID, A + EVAL),
    ("eval ldx, empty", INVALID, A + EVAL),
    ("eval ldg", INVALID, A + EVAL),
    ("pending ldg", INVALID, P + EVAL),
    ("pending ok", OK, ""),
    ("joint n < 0", INVALID, J + EVAL_JOINT),
    ("joint xq NULL", INVALID, J + EVAL_JOINT),
    ("joint ok", OK, ""),
    ("max ok", OK, ""),
    ("max a_out alone, ldxo unused", OK, ""),
    ("max no output (first of three)", INVALID, M + NO_OUT),
    ("max n_starts 0 (first of three)", INVALID, M + STARTS),
    ("max n_starts 2^31", INVALID, M + STARTS),
    ("max n_starts 2^31 - 1", OK, ""),
    ("max ldx0 (first of two)", INVALID, M + LDX0),
    ("max ldxo", INVALID, M + LDXO),
    ("batch ok", OK, ""),
    ("batch no xb_out (first of two)", INVALID, B + "xb_out must be given"),
    ("batch n_starts 2^31", INVALID, B + STARTS),
    ("batch ldx0 (first of two)", INVALID, B + LDX0),
    ("batch ldxb", INVALID, B + "ldxb >= D"),
    ("jmax ok", OK, ""),
    ("jmax no output (first of two)", INVALID, MJ + NO_OUT),
    ("jmax n_starts 2^27", INVALID, MJ + STARTS_JOINT),
    ("jmax n_starts 2^27 - 1", OK, ""),
    ("jmax n_starts 0", INVALID, MJ + STARTS_JOINT),
    ("jmax ldx0 (first of three)", INVALID, MJ + LDX0),
    ("jmax ldxo (first of two)", INVALID, MJ + LDXO),
    ("jmax ldb", INVALID, MJ + LDB),
    ("jmax no best_x, ldb unused", OK, ""),
]


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_compiled_checks_say_what_the_entry_points_said(tmp_path):
    cxx = _cxx()
    if not cxx:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "acq_check_messages"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", CSRC,
           os.path.join(ROOT, "tests", "c_host", "acq_check_messages.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = [tuple(line.split("\t")) for line in out.split("\n") if line]
    assert [g[0] for g in got] == [w[0] for w in WANT]
    for g, w in zip(got, WANT):
        assert (g[0], int(g[1]), g[2]) == w
