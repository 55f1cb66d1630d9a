"""Golden vectors for the correspondence / depth sampler (sr_corres_sample) from the REAL reference
functions (read-only import; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_corres.py

Imports the reference's train/utils/io.py and calls sample_correspondence_and_depth (io.py:280-360)
after np.random.seed(s); that module imports cv2, tqdm and torchvision at the top and
datasets/imc2021.py imports h5py and natsort, none of which the sampler touches: whichever is
missing is registered as an empty stand-in module before the import.  IMC2021._png2coords /
_png2certainty (imc2021.py:68-75) are called unbound and the source grid follows imc2021.py:126-131
line by line.

Seeds: for each case the seeds are searched upward from SEED0[case]; the first one for which every
RandomState(s).random_sample(P * K) value lies >= 2^-22 from every edge of the CDF that
np.random.choice builds from the reference's own probabilities (tests/corres_ref.py reference_cdf)
is kept.  An exact-weight fp64 implementation then returns the reference's index for every stored
uniform (DESIGN.md "Correspondence sampling"), so the tests compare indices with no exclusions.
The sampled index itself is not returned by the reference: it is recomputed here by numpy's own
rule (searchsorted(cdf, u, 'right') on that CDF) and checked to reproduce the reference's sampled
coordinates bit for bit before it is stored (unfiltered numbering).

Cases (g13_corres.npz, prefix per case):
  grid    one pair, 48x64 map, K = 64, threshold 0.1; a quarter of the certainties at or below the
          threshold (exact zeros, exact float32(0.1), values in between); depth maps 37x53 and 41x29;
          ~10 % of coords_dst outside [-1, 1] (zero-padded and partial taps)
  chunks  75x117 map (M = 8775: several scan chunks and a ragged tail for any chunk size <= 4096),
          K = 64, threshold 0
  sparse  M = 1500 with three eligible entries (first, last, one in between), K = 32
  one     M = 1, K = 5
  png     a 24x40 uint16 x / y / conf triple, the decoded arrays, K = 32, threshold 0.1
  multi   five pairs over three views reusing the arrays above (M and the depth sizes differ per
          pair), K = 32, threshold 0.05, one seed, uniforms consumed pair after pair
"""

from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SFM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REF, "train"))
sys.dont_write_bytecode = True


def _stand_in(name: str, **attrs) -> None:
    try:
        __import__(name)
    except ImportError:
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod


_stand_in("cv2")
_stand_in("tqdm")
_stand_in("torchvision", transforms=types.ModuleType("torchvision.transforms"))
_stand_in("h5py")
_stand_in("natsort", natsorted=sorted)

from utils.io import sample_correspondence_and_depth  # noqa: E402
from datasets.imc2021 import IMC2021  # noqa: E402

import corres_ref as R  # noqa: E402

SEED0 = {"grid": 100, "chunks": 200, "sparse": 300, "one": 400, "png": 500, "multi": 600}


def depth_map(rng, h, w):
    return (1 + 4 * rng.random_sample((h, w))).astype(np.float32)


def inputs():
    rng = np.random.RandomState(13)
    d = {0: depth_map(rng, 37, 53), 1: depth_map(rng, 41, 29), 2: depth_map(rng, 19, 23)}
    c = {}
    # grid
    m = 48 * 64
    cert = (0.11 + 0.89 * rng.random_sample(m)).astype(np.float32)
    low =rng.permutation(m)[: m // 4]
    cert[low[0::3]] = 0.0
    cert[low[1::3]] = np.float32(0.1)
    cert[low[2::3]] = (0.1 * rng.random_sample(low[2::3].size)).astype(np.float32)
    c["grid"] = dict(coords_src=R.grid(48, 64), coords_dst=rng.uniform(-1.06, 1.06, (m, 2)).astype(np.float32),
                     certainty=cert, min_conf=0.1, K=64)
    # chunks
    m = 75 * 117
    c["chunks"] = dict(coords_src=R.grid(75, 117), coords_dst=rng.uniform(-1.02, 1.02, (m, 2)).astype(np.float32),
                       certainty=(0.001 + rng.random_sample(m)).astype(np.float32), min_conf=0.0, K=64)
    # sparse
    m = 1500
    cert = (0.04 * rng.random_sample(m)).astype(np.float32)
    cert[[0, 777, 1499]] = np.float32([0.5, 0.9, 0.3])
    c["sparse"] = dict(coords_src=rng.uniform(-1, 1, (m, 2)).astype(np.float32),
                       coords_dst=rng.uniform(-1, 1, (m, 2)).astype(np.float32), certainty=cert, min_conf=0.05, K=32)
    # one
    c["one"] = dict(coords_src=np.float32([[0.25, -0.5]]), coords_dst=np.float32([[-0.125, 0.75]]),
                    certainty=np.float32([0.7]), min_conf=0.0, K=5)
    # png: decode with the reference's own methods, grid by imc2021.py:126-131
    hs, ws = 24, 40
    x_png = rng.randint(0, 65536, (hs, ws)).astype(np.uint16)
    y_png = rng.randint(0, 65536, (hs, ws)).astype(np.uint16)
    conf_png = rng.randint(0, 1001, (hs, ws)).astype(np.uint16)
    conf_png[rng.random_sample((hs, ws)) < 0.15] = 0
    conf_png[3, 5] = 100  # float32(100 / 1000) against the threshold float32(0.1): not eligible
    coordsjx = IMC2021._png2coords(None, x_png)
    coordsjy = IMC2021._png2coords(None, y_png)
    certainty = IMC2021._png2certainty(None, conf_png)
    coords_dst = np.stack([coordsjx, coordsjy], axis=-1)
    xx, yy = np.meshgrid(
        np.linspace(-1 + 1 / ws, 1 - 1 / ws, ws),
        np.linspace(-1 + 1 / hs, 1 - 1 / hs, hs),
        indexing="xy"
    )
    coords_src = np.stack([xx, yy], axis=-1)
    c["png"] = dict(x_png=x_png, y_png=y_png, conf_png=conf_png,
                    coords_src=coords_src.astype(np.float32).reshape(-1, 2),  # imc2021.py:307
                    coords_dst=coords_dst.astype(np.float32).reshape(-1, 2),
                    certainty=certainty.astype(np.float32).reshape(-1), min_conf=0.1, K=32)
    return d, c


def find_seed(start, pairs, K):
    """pairs: [(certainty, min_conf)].  First seed whose P * K uniforms keep the margin for every pair."""
    s = start
    while True:
        u = np.random.RandomState(s).random_sample(len(pairs) * K).reshape(len(pairs), K)
        if all(R.edge_margin(cert, u[j], mc) >= R.MARGIN for j, (cert, mc) in enumerate(pairs)):
            return s, u
        s += 1


def run_pairs(seed, u, pairs, K):
    """pairs: [(coords_src, coords_dst, certainty, depth_src, depth_dst, min_conf)] -> stacked outputs."""
    np.random.seed(seed)
    outs = []
    for j, (cs, cd, cert, ds, dd, mc) in enumerate(pairs):
        a, b, e, f = sample_correspondence_and_depth(cs, cd, cert, ds, dd, K, mc)
        sel, cdf = R.reference_cdf(cert, mc)
        idx_f = cdf.searchsorted(u[j], side="right")
        index = np.flatnonzero(sel)[idx_f]
        assert np.array_equal(a, R.to_pixels(cs[index], *ds.shape)), "index does not reproduce the reference"
        assert np.array_equal(b, R.to_pixels(cd[index], *dd.shape))
        outs.append((index.astype(np.int32), a.astype(np.float32), b.astype(np.float32),
                     np.asarray(e, np.float32).reshape(K), np.asarray(f, np.float32).reshape(K)))
    assert np.random.random_sample() == np.random.RandomState(seed).random_sample(len(pairs) * K + 1)[-1]
    return [np.stack(t) for t in zip(*outs)]


def main():
    depths, cases = inputs()
    out = {}
    for v, dm in depths.items():
        out[f"depth_{v}"] = dm
    for name, c in cases.items():
        K = c["K"]
        seed, u = find_seed(SEED0[name], [(c["certainty"], c["min_conf"])], K)
        index, a, b, e, f = run_pairs(seed, u, [(c["coords_src"], c["coords_dst"], c["certainty"], depths[0],
                                                  depths[1], c["min_conf"])], K)
        for k, v in c.items():
            out[f"{name}/{k}"] = np.asarray(v)
        out[f"{name}/seed"] = np.int64(seed)
        out[f"{name}/uniforms"] = u[0]
        out[f"{name}/src_view"], out[f"{name}/dst_view"] = np.int64(0), np.int64(1)
        out[f"{name}/index"], out[f"{name}/out_src_coords"], out[f"{name}/out_dst_coords"] = index[0], a[0], b[0]
        out[f"{name}/out_src_depth"], out[f"{name}/out_dst_depth"] = e[0], f[0]
        print(f"{name}: seed {seed} (searched from {SEED0[name]}), M {c['certainty'].size}, eligible "
              f"{int(R.reference_cdf(c['certainty'], c['min_conf'])[0].sum())}, margin "
              f"{R.edge_margin(c['certainty'], u[0], c['min_conf']):.3e}")
    # multi: five pairs over three views, the arrays above
    corr_from = ["grid", "chunks", "sparse", "one", "png"]
    views = [(0, 1), (1, 2), (2, 0), (1, 0), (2, 2)]
    K, mc = 32, 0.05
    seed, u = find_seed(SEED0["multi"], [(cases[n]["certainty"], mc) for n in corr_from], K)
    index, a, b, e, f = run_pairs(seed, u, [(cases[n]["coords_src"], cases[n]["coords_dst"], cases[n]["certainty"],
                                             depths[s], depths[t], mc) for n, (s, t) in zip(corr_from, views)], K)
    out["multi/corr_from"] = np.array(corr_from)
    out["multi/src_view"] = np.int64([s for s, _ in views])
    out["multi/dst_view"] = np.int64([t for _, t in views])
    out["multi/min_conf"], out["multi/K"], out["multi/seed"], out["multi/uniforms"] = mc, K, np.int64(seed), u
    out["multi/index"], out["multi/out_src_coords"], out["multi/out_dst_coords"] = index, a, b
    out["multi/out_src_depth"], out["multi/out_dst_depth"] = e, f
    print(f"multi: seed {seed} (searched from {SEED0['multi']})")
    path = os.path.join(HERE, "g13_corres.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
