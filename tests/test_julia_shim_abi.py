"""Every `ccall` of the Julia shim (julia/AGPHip.jl) names a function of include/agp_hip.h and passes as many arguments as the
prototype declares.  Julia is not needed: the shim and the header are parsed as text."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _split_top(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "({[":
            depth += 1
        elif ch in ")}]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _close(s, i):
    """index just past the bracket group that opens at s[i]"""
    depth = 0
    for j in range(i, len(s)):
        if s[j] in "({[":
            depth += 1
        elif s[j] in ")}]":
            depth -= 1
            if depth == 0:
                return j + 1
    raise ValueError("unbalanced")


def header_prototypes():
    h = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    protos = {}
    for m in re.finditer(r"^\s*(?:agp_status|int32_t|const char\*)\s+(agp_\w+)\s*\(", h, flags=re.M):
        j = _close(h, m.end() - 1)
        params = h[m.end():j - 1].strip()
        protos[m.group(1)] = 0 if params in ("", "void") else len(_split_top(params))
    return protos


def shim_ccalls():
    s = open(os.path.join(ROOT, "julia", "AGPHip.jl")).read()
    calls = []
    for m in re.finditer(r"ccall\(\(:(\w+),\s*libagp\)\s*,", s):
        i = m.end()
        ret_end = i
        depth = 0
        while True:  # the return type: up to the next top-level comma
            ch = s[ret_end]
            if ch in "({[":
                depth += 1
            elif ch in ")}]":
                depth -= 1
            elif ch == "," and depth == 0:
                break
            ret_end += 1
        k = ret_end + 1
        while s[k].isspace():
            k += 1
        assert s[k] == "(", (m.group(1), s[k:k + 40])
        tup = s[k + 1:_close(s, k) - 1]
        calls.append((m.group(1), len(_split_top(tup))))
    return calls


def test_every_ccall_matches_the_header():
    protos = header_prototypes()
    calls = shim_ccalls()
    assert len(calls) > 60 and len(protos) > 60
    bad = [(n, k, protos.get(n)) for n, k in calls if protos.get(n) != k]
    assert not bad, bad


def test_shim_creates_full_handles_for_vgp():
    s = open(os.path.join(ROOT, "julia", "AGPHip.jl")).read()
    assert "const AGP_FLAG_FULL = Int32(2)" in s and "AGP.VGP{T,<:Any,<:AnalyticVI}" in s
