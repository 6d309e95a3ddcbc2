"""Every header under csrc/ compiles on its own: it includes what it uses.  agp_capi.hip is one translation unit that includes
them all in a fixed order, so a header that leans on what happened to be included before it would never be noticed there.
Cross-compiles for gfx950 without a GPU (-fsyntax-only, host and device pass); reads and compiles the headers, nothing more."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgaussianprocesses.jl_amd", "csrc")
HEADERS = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.h")))


def _hipcc():
    h = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return h if os.path.exists(h) else shutil.which("hipcc")


def test_the_headers_are_found():  # (an empty parametrisation below would pass by running nothing)
    assert "agp_ctx.h" in HEADERS and "agp_svgp_base.h" in HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc on this machine")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-Wno-pragma-once-outside-header", "-x", "hip",
           os.path.join(CSRC, header)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{header} does not compile on its own:\n{r.stderr[-4000:]}"
