"""The routes through hmsc_krige and hmsc_predict_map's kriging, one line each: a SHA-256 of the output
bytes, or -- for a refused route -- the return code / exception and the message.  Run on two builds on
the same machine, the listings must be identical (profiles/krige_plan_paths*.txt).

    python scripts/krige_paths.py > listing.txt

Inputs from tests/krige_cases.py, gpp_cases.py and map_cases.py: 70 fitted units, up to 150 new, 37
species, 9 samples.  hmsc_krige is called on raw arguments (every refusal is reachable there); the maps go
through predictMap, a refusal route editing the level's description on its way to the device call."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import map_cases as MC  # noqa: E402
from helpers import H  # noqa: E402
from hmsc_amd import _lib as L  # noqa: E402
from hmsc_amd import gradient as GR  # noqa: E402

NP, S, NF = MC.NP, MC.NSAMP, 3
PROBS = (0.1, 0.5)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def line(name, text):
    print(f"{name:58s} {text}", flush=True)


# ---- hmsc_krige on raw arguments ---------------------------------------------------------------

def posterior(npo, S=S, nf=NF, seed=5):
    """Eta (S x nf x np) and the grid indices: map_cases' cycle (index 1 is a = 0, so some pairs sit at
    a = 0), every third sample's last factor zero padded."""
    rng = np.random.default_rng(seed)
    eta = rng.standard_normal((S, nf, npo))
    idx = np.array([[MC.ALPHA_IDX[(nf * s + h) % len(MC.ALPHA_IDX)] for h in range(nf)] for s in range(S)], dtype=np.int32)
    idx[::3, nf - 1] = 0
    eta[::3, nf - 1] = 0.0
    return eta, idx


def krige(mode, nn, npo=NP, dist=False, timed=False, eta_idx=None, k=5, seed=11, edit=None, alphas=MC.GRID):
    xy = np.random.default_rng(100 + nn).random((npo + nn, 2))
    eta, idx = posterior(npo) if eta_idx is None else eta_idx
    knots = np.asarray(H.constructKnots(xy[:npo], nKnots=3), dtype=np.float64)
    d = dict(xy=xy, knots=knots, idx=idx.copy(), nNeighbours=k, nK=len(knots), dist=dist, null_knots=False)
    if edit:
        edit(d)
    keep = []
    a = L.hmsc_krige_args()
    a.device, a.np, a.nn, a.G, a.S, a.nfmax, a.mode, a.level = 0, npo, nn, len(alphas), eta.shape[0], eta.shape[1], mode, 1
    a.nNeighbours, a.seed = d["nNeighbours"], seed
    if d["dist"]:
        D = np.sqrt(((d["xy"][:, None, :] - d["xy"][None, :, :]) ** 2).sum(-1))
        a.dist, a.sDim = L.colmajor_ptr(D, keep), 0
    else:
        a.coords, a.sDim = L.colmajor_ptr(d["xy"], keep), 2
    if mode == 4:
        a.knots, a.nK = (None if d["null_knots"] else L.colmajor_ptr(d["knots"], keep)), d["nK"]
    al, e, ix = np.ascontiguousarray(alphas, dtype=np.float64), np.ascontiguousarray(eta), np.ascontiguousarray(d["idx"])
    a.alphas, a.Eta, a.alpha = L.fptr(al), L.fptr(e), L.iptr(ix)
    ms = np.zeros(8)
    if timed:
        a.kernel_ms = L.fptr(ms)
    out = np.full((eta.shape[0], eta.shape[1], nn), np.nan)
    rc = L.lib().hmsc_krige(C.byref(a), L.fptr(out))
    return sha(out) if rc == 0 else f"rc={rc} {L.lib().hmsc_last_error().decode()}"


def krige_routes():
    for mode in range(5):
        for nn in (1, 64, 70):
            line(f"krige mode={mode} nn={nn} coords", krige(mode, nn))
        line(f"krige mode={mode} nn=70 coords kernel_ms", krige(mode, 70, timed=True))
        if mode < 3:
            line(f"krige mode={mode} nn=70 dist", krige(mode, 70, dist=True))
    rng = np.random.default_rng(8)     # 130 of 140 pairs on one grid value: two 64-column tiles
    idx = np.full((70, 2), 5, dtype=np.int32)
    for s in range(5):
        idx[7 * s, s % 2] = 3 + s % 2
    many = (rng.standard_normal((70, 2, NP)), idx)
    for mode in range(5):
        line(f"krige mode={mode} nn=5 130 pairs on one grid value", krige(mode, 5, eta_idx=many))
    eta, idx = posterior(NP)
    zero = (eta, np.where(idx > 0, 1, 0).astype(np.int32))
    for mode in (0, 2, 3, 4):
        line(f"krige mode={mode} nn=70 every pair at a = 0", krige(mode, 70, eta_idx=zero))
    # refusals
    def grid9(d):
        d["idx"][1, 0] = 9

    line("krige refused: grid index out of range", krige(1, 3, edit=grid9))
    for k in (0, 33):
        line(f"krige refused: nNeighbours={k}", krige(3, 3, k=k))
    line("krige refused: nNeighbours=21 > np=20", krige(3, 3, npo=20, k=21))
    line("krige refused: mode 3 with dist", krige(3, 3, dist=True))
    line("krige refused: mode 4 with dist", krige(4, 3, dist=True))
    line("krige refused: mode 4 nK=0", krige(4, 3, edit=lambda d: d.update(nK=0)))
    line("krige refused: mode 4 NULL knots", krige(4, 3, edit=lambda d: d.update(null_knots=True)))
    def on_knot(d):
        d["knots"][2] = d["xy"][5]

    line("krige refused: mode 4 fitted unit on a knot", krige(4, 3, edit=on_knot))
    def twins(d):
        d["xy"][NP + 1] = d["xy"][NP]

    line("krige refused: mode 2 coincident new units", krige(2, 3, edit=twins))
    def nan(d):
        d["xy"][NP + 1, 0] = np.nan

    line("krige refused: mode 3 non-finite coordinates", krige(3, 3, edit=nan))


# ---- hmsc_predict_map through predictMap ---------------------------------------------------------

MODES = {"mean": ("Full", dict(predictEtaMean=True)), "field": ("Full", dict(predictEtaMeanField=True)),
         "full": ("Full", dict()), "nngp": ("NNGP", dict()), "gpp": ("GPP", dict(gppDevice=True))}
_models = {}


def model(method):
    if method not in _models:
        hM = MC.model(method, **(dict(nNeighbours=5) if method == "NNGP" else dict(sKnot="auto") if method == "GPP" else {}))
        _models[method] = (hM, MC.posterior(hM))
    return _models[method]


def map_sha(res):
    parts = []
    for part, keys in (("cells", ("n", "occ", "mean", "quantiles")), ("community", ("n", "mean", "quantiles"))):
        if res[part] is not None:
            parts += [np.asarray(res[part][k]) for k in keys]
    return sha(*parts)


def pmap(mode, G=None, nn=150, slab_rows=64, post=None, edit=None, no_python_slab_check=False, **kw):
    method, mkw = MODES[mode]
    hM, p = model(method)
    w = np.zeros(hM.ns)
    w[4] = 1.0
    real_level, real_plan = GR._map_level, GR.map_slab_plan

    def level(*a, **k):
        lev = real_level(*a, **k)
        if edit and lev["name"] == "plot":
            edit(lev)
        return lev

    GR._map_level = level
    if no_python_slab_check:
        GR.map_slab_plan = lambda *a, **k: []
    try:
        args = dict(post=post or p, seed=17, expected=False, probs=PROBS, measures=("S", "T"), weights={"sp4": w},
                    slab_rows=slab_rows, **mkw)
        args.update(kw)
        if "studyDesign" not in args:
            args["Gradient"] = G or MC.grid(hM, nn)
        return map_sha(H.predictMap(hM, **args))
    except Exception as e:  # a refusal: its type and text
        return f"{type(e).__name__}: {e}"
    finally:
        GR._map_level, GR.map_slab_plan = real_level, real_plan


def mixed_design(hM, only_fitted_spatial):
    """100 rows at fitted and new units of both levels in no order (test_gpu_predict_map's); or the
    spatial level at fitted units only beside new non-spatial ones."""
    rng = np.random.default_rng(3)
    n_new, rows = 30, 100
    names = [f"p{k:03d}" for k in range(MC.NP)] + [f"q{k:03d}" for k in range(n_new)]
    rl = hM.rL[0].copy()
    rl.s = np.vstack([np.asarray(rl.s, dtype=np.float64), rng.random((n_new, 2))])
    rl["sNames"] = names
    rl.pi = names
    rl.N = len(names)
    sites = [f"u{k:02d}" for k in range(MC.NSITE)] + ["z1", "z2"]
    plots = names[:MC.NP] if only_fitted_spatial else names
    sd = pd.DataFrame({"plot": rng.choice(plots, rows), "site": rng.choice(sites, rows)})
    X = np.column_stack([np.ones(rows), rng.standard_normal((rows, 2))])
    return dict(X=X, studyDesign=sd, ranLevels={"plot": rl, "site": hM.rL[1]})


def map_routes():
    for mode in ("mean", "field", "nngp", "gpp"):
        for rows in (64, 128, 0):
            line(f"map {mode} nn=150 slab_rows={rows}", pmap(mode, slab_rows=rows))
    for rows in (0, 64):
        line(f"map full nn=40 slab_rows={rows}", pmap("full", nn=40, slab_rows=rows))
    for mode in ("field", "nngp", "gpp"):
        hM, _ = model(MODES[mode][0])
        G = MC.shared_units(MC.grid(hM, 150), ((20, 120), (3, 149)))
        line(f"map {mode} shared units slab_rows=64", pmap(mode, G=G))
    for mode in ("field", "gpp"):
        hM, _ = model(MODES[mode][0])
        for rows in (64, 0):
            line(f"map {mode} fitted and new units mixed slab_rows={rows}",
                 pmap(mode, slab_rows=rows, **mixed_design(hM, False)))
            line(f"map {mode} spatial level without new units slab_rows={rows}",
                 pmap(mode, slab_rows=rows, **mixed_design(hM, True)))
    hM, post = model("GPP")
    zero = [dict(s, Alpha=[np.ones_like(s["Alpha"][0]), s["Alpha"][1]]) for s in post]
    for rows in (64, 0):
        line(f"map gpp every pair at a = 0 slab_rows={rows}", pmap("gpp", post=zero, slab_rows=rows))
    line("map field one slab of 100 rows", pmap("field", nn=100, slab_rows=0))
    # refusals
    def grid9(lev):
        lev["alpha"][1, 0] = 9

    line("map refused: grid index out of range", pmap("field", edit=grid9))
    for k in (0, 33):
        line(f"map refused: nNeighbours={k}", pmap("nngp", edit=lambda lev, k=k: lev.update(nNeighbours=k)))
    def by_dist(lev):
        xy = lev["coords"]
        lev.update(dist=np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)), coords=None, sDim=0)
    line("map refused: mode 3 with dist", pmap("nngp", edit=by_dist))
    line("map refused: mode 4 with dist", pmap("gpp", edit=by_dist))
    line("map refused: mode 4 without knots", pmap("gpp", edit=lambda lev: lev.update(knots=None)))
    def on_knot(lev):
        lev["knots"] = np.vstack([lev["coords"][5], lev["knots"][1:]])

    line("map refused: mode 4 fitted unit on a knot", pmap("gpp", edit=on_knot))
    def twins(lev):
        lev["coords"][MC.NP + 1] = lev["coords"][MC.NP]

    line("map refused: full coincident new units", pmap("full", nn=40, slab_rows=0, edit=twins))
    def nan(lev):
        lev["coords"][MC.NP + 1, 0] = np.nan

    line("map refused: nngp non-finite coordinates", pmap("nngp", edit=nan))
    line("map refused: full spread over slabs (python)", pmap("full", nn=150, slab_rows=64))
    line("map refused: full spread over slabs (native)", pmap("full", nn=150, slab_rows=64, no_python_slab_check=True))
    for mode in MODES:
        line(f"map refused: {mode} factor_bytes=1024", pmap(mode, nn=40, slab_rows=64 if mode != "full" else 0, factor_bytes=1024))


if __name__ == "__main__":
    krige_routes()
    map_routes()
