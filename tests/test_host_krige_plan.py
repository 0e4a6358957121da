"""The pure part of the kriging level plan (hmsc_amd/csrc/krige_level.h: krige_group_pairs,
krige_check_mode, krige_need_bytes) on the host: tests/capi/krige_plan_check.cpp is built with the
library's flags plus AddressSanitizer and UBSan and run as a program of its own (no device, nothing
loaded into Python), and its output is held to a numpy restatement of the grouping and of the two
device-memory formulas as hmsc_krige (capi.cpp) and run_predict_map (map.hip) had them before both
moved onto the plan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from hmsc_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "capi", "krige_plan_check.cpp")
DENSE_SYNC_INTS = 2 + 4096 + 2                     # state.h
ALPHAS = [0.0, 0.05, 0.4, 1.1]                     # index 1 is a = 0

pytestmark = pytest.mark.skipif(not (os.path.exists(B.HIPCC) or shutil.which(B.HIPCC)), reason="no hipcc")


def dense_ws(n):
    return (n + 63) // 64 * 64 * 64 + n + 64


def gpp_plan(npo, nK, c):
    return 3 * nK * nK + npo * nK + npo + npo * c + 2 * nK * c + dense_ws(nK)


class Refused(Exception):
    pass


def _by_grid(q):
    """(s, h) pairs by grid index; 'GPP' files a sample's factors under its last factor's index."""
    S, nf, G = q["alpha"].shape[0], q["alpha"].shape[1], len(q["alphas"])
    by_g = [[] for _ in range(G + 1)]
    for s in range(S):
        glast = 0
        for h in range(nf):
            g = int(q["alpha"][s, h])
            if not 0 <= g <= G:
                raise Refused(f"grid index {g} of sample {s}, factor {h} is outside the alphapw grid 1..{G}")
            if g > 0:
                glast = g
        for h in range(nf):
            g = int(q["alpha"][s, h])
            if g > 0:
                by_g[glast if q["mode"] == 4 else g].append(s * nf + h)
    return by_g


def _check_mode(q):
    if q["mode"] == 3:
        if not q["coords"]:
            raise Refused("NNGP kriging needs coordinates; a distMat level predicts with 'Full'")
        if q["nNeighbours"] < 1:
            raise Refused("nNeighbours must be positive")
        if q["nNeighbours"] > 32:
            raise Refused(f"NNGP kriging on the device takes nNeighbours <= 32 (got {q['nNeighbours']})")
        if q["nNeighbours"] > q["np"]:
            raise Refused("nNeighbours exceeds the number of fitted units")
    if q["mode"] == 4:
        if not q["coords"] or q["dist"]:
            raise Refused("GPP kriging needs coordinates; a distMat level predicts with 'Full'")
        if not q["knots"] or q["nK"] <= 0:
            raise Refused("GPP kriging needs knots (knots with nK > 0)")


def _groups(q, by_g, keep):
    nf = q["alpha"].shape[1]
    out = dict(g_idx=[], g_alpha=[], g_off=[0], col_s=[], col_h=[], cmax=0)
    for g in range(1, len(by_g)):
        if not by_g[g] or not keep(g):
            continue
        out["col_s"] += [p // nf for p in by_g[g]]
        out["col_h"] += [p % nf for p in by_g[g]]
        out["g_idx"].append(g)
        out["g_alpha"].append(q["alphas"][g - 1])
        out["g_off"].append(len(out["col_s"]))
        if q["alphas"][g - 1] > 0:
            out["cmax"] = max(out["cmax"], len(by_g[g]))
    return out


def krige_reference(q):
    """hmsc_krige before the plan: the mode's checks, every group kept, the call's bytes."""
    _check_mode(q)
    g = _groups(q, _by_grid(q), lambda g: True)
    npo, nn, S, nf, nK, cmax = q["np"], q["nn"], q["alpha"].shape[0], q["alpha"].shape[1], q["nK"], g["cmax"]
    N, gpp = npo + nn, q["mode"] == 4
    nK = nK if gpp else 0
    dense = q["mode"] != 3 and not gpp and cmax > 0
    need = (N * N if not q["coords"] else N * q["sDim"]) + S * npo * nf + S * nn * nf
    if dense:
        need += npo * npo + npo * (nn + cmax) + dense_ws(npo)
        if q["mode"] == 1:
            need += nn
        if q["mode"] == 2:
            need += nn * nn + nn * cmax + dense_ws(nn)
    if gpp:
        need += nK * q["sDim"]
    if gpp and cmax > 0:
        need += gpp_plan(npo, nK, cmax) + nK * nK + nK * cmax + nn
    ipg = 4 if gpp else 2
    g["need"] = need * 8 + (2 * len(g["col_s"]) + (ipg + 1) * len(g["g_idx"]) + 2 + DENSE_SYNC_INTS) * 4
    return g


def map_reference(q, mmax, ns=7, Umax=50, nunits=120):
    """A level of run_predict_map before the plan: the groups at a = 0 left to the assembly kernel's zflag
    (mode 3 keeps them, its kernel writes z), no groups without new units, the checks when a group
    needs them; the level's bytes less the map's own share (Lambda, the Eta table, the unit lists, zflag)."""
    S, nf = q["alpha"].shape
    by_g = _by_grid(q)
    zflag = np.zeros(S * nf, dtype=int)
    for g in range(1, len(by_g)):
        if not q["alphas"][g - 1] > 0 and q["mode"] != 0:
            zflag[by_g[g]] = 1
    g = _groups(q, by_g, lambda g: q["alphas"][g - 1] > 0 or q["mode"] == 3)
    if g["cmax"] > 0 and not (q["coords"] or q["dist"]):
        raise Refused("a grid value > 0 needs coords or dist")
    if q["nn"] == 0:
        g = dict(g_idx=[], g_alpha=[], g_off=[0], col_s=[], col_h=[], cmax=0)
    if q["mode"] == 3:
        zflag[:] = 0
    if q["mode"] == 3 and g["g_idx"] or q["mode"] == 4 and g["cmax"] > 0:
        _check_mode(q)
    gpp = q["mode"] == 4 and g["cmax"] > 0
    dense = q["mode"] not in (3, 4) and g["cmax"] > 0
    full = dense and q["mode"] == 2
    npo, nn, nK, cmax = q["np"], q["nn"], q["nK"], g["cmax"]
    N = npo + nn
    cols = [g["g_off"][k + 1] - g["g_off"][k] for k in range(len(g["g_idx"]))]
    dbl = S * npo * nf + S * nf * ns + S * Umax * nf
    if g["g_idx"]:
        dbl += N * q["sDim"] if q["coords"] else N * N
    if dense and not full:
        pos = [c for c, a in zip(cols, g["g_alpha"]) if a > 0]
        dbl += len(pos) * (npo * npo + dense_ws(npo)) + npo * sum(pos)
        dbl += npo * mmax + mmax
    if gpp:
        dbl += nK * q["sDim"] + gpp_plan(npo, nK, cmax) + mmax
        dbl += sum(nK * nK + nK * c for c, a in zip(cols, g["g_alpha"]) if a > 0)
    if full:
        dbl += npo * npo + npo * (nn + cmax) + dense_ws(npo) + nn * nn + nn * cmax + dense_ws(nn)
    total = dbl * 8 + (2 * nunits + 2 * len(g["col_s"]) + S * nf + 6 * len(g["g_idx"]) + 2 + DENSE_SYNC_INTS) * 4
    g["need"] = total - ((S * nf * ns + S * Umax * nf) * 8 + (2 * nunits + S * nf) * 4)
    g["zflag"] = list(zflag)
    return g


def spec(keep_zero, mode, nn=40, slab=24, alpha=((2, 3, 1), (3, 0, 0), (4, 2, 3)), coords=1, dist=0, knots=None,
         nK=None, k=5, npo=70):
    gpp = mode == 4
    return dict(keep_zero=keep_zero, slab=slab, mode=mode, np=npo, nn=nn, sDim=2 if coords else 0,
                nK=(16 if gpp else 0) if nK is None else nK, nNeighbours=k, alphas=ALPHAS, alpha=np.array(alpha),
                coords=coords, dist=dist, knots=(1 if gpp else 0) if knots is None else knots)


# each mode on both clients; the GPP last-factor rule with a zero-padded sample (sample 1: its only
# factor, sample 0: filed under index 1, a = 0, although two factors sit at a > 0); a = 0 groups kept
# (hmsc_krige) and dropped (the map); a level without new units; a distMat level; every pair at a = 0
SPECS = [spec(kz, mode) for mode in range(5) for kz in (1, 0)] + [
    spec(0, 1, nn=0), spec(0, 4, nn=0), spec(1, 2, coords=0, dist=1), spec(0, 0, coords=0, dist=1),
    spec(1, 4, alpha=((1, 1, 1), (1, 0, 0))), spec(0, 4, alpha=((1, 1, 1), (1, 0, 0))),
    spec(1, 1, alpha=((3, 3, 3), (3, 3, 0), (3, 2, 3))), spec(0, 2, alpha=((3, 3, 3), (3, 3, 0), (3, 2, 3)), slab=40),
]
BAD = [spec(1, 1, alpha=((2, 5, 1),)), spec(0, 1, alpha=((2, 5, 1),)), spec(1, 3, k=33), spec(0, 3, k=0),
       spec(1, 3, k=21, npo=20), spec(1, 4, coords=0, dist=1), spec(0, 4, knots=0), spec(1, 4, nK=0),
       spec(0, 3, coords=0, dist=1), spec(0, 1, coords=0, dist=0)]


def _line(q):
    head = [q["keep_zero"], q["slab"], q["mode"], q["np"], q["nn"], q["sDim"], q["nK"], q["nNeighbours"], len(q["alphas"]),
            q["alpha"].shape[0], q["alpha"].shape[1], q["coords"], q["dist"], q["knots"]]
    return " ".join(map(str, head)) + " | " + " ".join(map(repr, q["alphas"])) + " | " + \
        " ".join(str(int(v)) for v in q["alpha"].ravel())


def _parse(text):
    blocks = [b.strip().splitlines() for b in text.split("spec\n")[1:]]
    out = []
    for b in blocks:
        if b[0].startswith("refused "):
            out.append(b[0][len("refused "):])
            continue
        d = {}
        for ln in b:
            name, *vals = ln.split()
            d[name] = [float(v) if name == "g_alpha" else int(v) for v in vals]
        d["cmax"], d["need"] = d["cmax"][0], d["need"][0]
        out.append(d)
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("krige_plan") / "krige_plan_check")
    cmd = [B.HIPCC] + B.FLAGS + ["-Xarch_host", "-fsanitize=address,undefined", "-x", "hip", SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def _run(program, specs):
    r = subprocess.run([program], input="\n".join(_line(q) for q in specs) + "\n", capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])     # (a sanitizer report is on stderr)
    got = _parse(r.stdout)
    assert len(got) == len(specs)
    return got


def test_groups_and_needs(program):
    for q, got in zip(SPECS, _run(program, SPECS)):
        ref = krige_reference(q) if q["keep_zero"] else map_reference(q, q["slab"])
        assert isinstance(got, dict), (q, got)
        for key in ("g_idx", "g_alpha", "g_off", "col_s", "col_h", "cmax", "need"):
            assert got[key] == ref[key], (key, q, got[key], ref[key])
        if not q["keep_zero"]:
            assert got["zflag"] == ref["zflag"], (q, got["zflag"], ref["zflag"])
    # the specs reach what they are for
    refs = [krige_reference(q) if q["keep_zero"] else map_reference(q, q["slab"]) for q in SPECS]
    assert any(r["cmax"] == 0 and r["g_idx"] for r in refs) and any(not r["g_idx"] for r in refs)
    assert any(1 in r["g_idx"] for r in refs) and any(sum(r.get("zflag", [])) > 0 for r in refs)


def test_refusals(program):
    for q, got in zip(BAD, _run(program, BAD)):
        with pytest.raises(Refused) as e:
            krige_reference(q) if q["keep_zero"] else map_reference(q, q["slab"])
        assert got == "check: " + str(e.value), (q, got)
