"""Correspondence / depth sampler (sr_corres_sample; train/utils/io.py:280-360 per pair), CPU side:
the fp64 restatement of its contract (tests/corres_ref.py) against the reference's goldens
(tests/golden/make_golden_corres.py -> g13_corres.npz), the margin condition that makes index
equality hold with no exclusions, the uint16 decode and the linspace grid, the ctypes mirror of the
new ABI structs, and the argument checks of the two Python entry points (no GPU is touched).

Depths: the reference's are fp32 grid_sample results, the restatement's an fp64 bilinear of the same
fp32 coordinates.  An fp32 evaluation rounds the pixel position (half an ulp of x <= 53, times a
depth slope of up to 4 per pixel: ~1e-5), so the two must agree to 2.5e-5 = a quarter of 1e-4 on
these maps (depths in [1, 5]) if they read the same four taps, zero-padded ones included, and
differ by O(1) if they do not.  The bound the GPU test uses, max(4 * max|golden - fp64|, 2 fp32 ulps),
is derived from that difference (corres_ref.depth_bound) and asserted here to stay below 1e-4.
"""

import ctypes
import json
import os
import subprocess
import threading

import numpy as np
import pytest
import torch

import corres_ref as R
from conftest import REPO


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_matches_reference(name):
    c, o = R.case(name), R.oracle(name)
    for j, (idx, sc, dc, sd, dd) in enumerate(o):
        assert np.array_equal(idx, c["index"][j]), (name, j)  # none excluded
        assert sc.dtype == np.float32 and np.array_equal(sc, c["out_src_coords"][j])  # bit-equal
        assert dc.dtype == np.float32 and np.array_equal(dc, c["out_dst_coords"][j])
        assert idx.max() < c["pairs"][j]["certainty"].size
    bound = R.depth_bound(name)
    print(f"{name}: depth bound {bound:.3e}")
    assert bound < 1e-4


@pytest.mark.parametrize("name", R.CASES)
def test_uniforms_keep_the_margin(name):
    """Every stored uniform lies >= 2^-22 from every edge of the reference's own CDF, and the stored
    uniforms are RandomState(seed).random_sample(P * K), consumed pair after pair."""
    c = R.case(name)
    P, K = c["uniforms"].shape
    assert K == c["K"] and P == len(c["pairs"])
    assert np.array_equal(np.random.RandomState(c["seed"]).random_sample(P * K).reshape(P, K), c["uniforms"])
    for j, p in enumerate(c["pairs"]):
        assert R.edge_margin(p["certainty"], c["uniforms"][j], c["min_conf"]) >= R.MARGIN, (name, j)


def test_cases_exercise_their_risks():
    g = R.case("grid")["pairs"][0]
    cert = g["certainty"]
    assert 0.2 < (cert <= np.float32(0.1)).mean() < 0.3 and (cert == 0).any() and (cert == np.float32(0.1)).any()
    assert 0.05 < (np.abs(g["coords_dst"]) > 1).any(axis=1).mean() < 0.2
    assert g["depth_src"].shape == (37, 53) and g["depth_dst"].shape == (41, 29)
    assert R.case("chunks")["pairs"][0]["certainty"].size == 75 * 117
    s = R.case("sparse")
    assert np.flatnonzero(s["pairs"][0]["certainty"] > np.float32(s["min_conf"])).tolist() == [0, 777, 1499]
    assert set(np.unique(s["index"])) == {0, 777, 1499}
    assert R.case("one")["pairs"][0]["certainty"].size == 1 and R.case("one")["K"] == 5
    m = R.case("multi")
    assert len(m["pairs"]) == 5 and len({p["certainty"].size for p in m["pairs"]}) == 5
    assert len({(p["depth_src"].shape, p["depth_dst"].shape) for p in m["pairs"]}) == 5
    assert os.path.getsize(R.GOLDEN) < 512 * 1024


def test_png_decode_and_grid_bit_equal():
    p = R.case("png")["pairs"][0]
    coords_dst, cert = R.decode_png(p["x_png"], p["y_png"], p["conf_png"])
    assert coords_dst.dtype == np.float32 and np.array_equal(coords_dst, p["coords_dst"])
    assert cert.dtype == np.float32 and np.array_equal(cert, p["certainty"])
    assert np.array_equal(R.grid(*p["conf_png"].shape), p["coords_src"])
    # the element-wise rule the kernel follows: i * step + start unfused, last element = stop
    for n in (24, 40, 1, 2, 117):
        start, stop = -1 + 1 / n, 1 - 1 / n
        ref = np.linspace(start, stop, n)
        step = (stop - start) / (n - 1) if n > 1 else 0.0
        mine = np.array([start if n == 1 else (stop if i == n - 1 else i * step + start) for i in range(n)])
        assert np.array_equal(ref, mine), n


def test_ctypes_mirror_of_the_corres_structs():
    """Field order and sizes of sr_corres_pair / sr_corres_desc as the header declares them (the C
    layout itself: abi_host_check `layout corres`, test below)."""
    from sailrecon_amd import _lib
    src = open(os.path.join(REPO, "include", "sfm_amd.h")).read()
    for cname, cls in (("sr_corres_pair", _lib.CorresPair), ("sr_corres_desc", _lib.CorresDesc)):
        body = src.split(f"typedef struct {cname} {{")[1].split(f"}} {cname};")[0]
        body = "\n".join(line.split("/*")[0] for line in body.splitlines())
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                names += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
        assert names == [f[0] for f in cls._fields_], cname
    assert ctypes.sizeof(_lib.CorresPair) == 80 and ctypes.sizeof(_lib.CorresDesc) == 112
    assert "sr_corres_sample" in _lib.EXPORTED and "sr_corres_sample_workspace" in _lib.EXPORTED
    lib = _lib.load()
    assert lib.sr_version() >= (1 << 16) | 6
    assert lib.sr_corres_sample_workspace(1, 1) >= 2 and lib.sr_corres_sample_workspace(0, 5) == 0
    got = []

    def rejected():  # on a thread of its own: sr_last_error is per thread, and test_abi.py expects it empty
        d = _lib.CorresDesc()
        got.append((lib.sr_corres_sample(None, ctypes.byref(d)), lib.sr_last_error()))

    t = threading.Thread(target=rejected)
    t.start()
    t.join()
    assert got[0][0] == -1 and b"sr_corres_sample" in got[0][1]


def test_ctypes_layout_matches_c():
    exe = os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "self-supervise-sfm_amd", "csrc"), "-j",
                        str(min(8, os.cpu_count() or 8)), "debug-build"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    lay = json.loads(subprocess.run([exe, "layout", "corres"], capture_output=True, text=True, env=env,
                                    check=True).stdout)
    for name, cls in (("sr_corres_pair", _lib.CorresPair), ("sr_corres_desc", _lib.CorresDesc)):
        assert ctypes.sizeof(cls) == lay[name]["size"]
        assert {f[0] for f in cls._fields_} == set(lay[name]["fields"])
        for f, off in lay[name]["fields"].items():
            assert getattr(cls, f).offset == off, (name, f)


# ---------------------------------------------------------------- argument checks (host side, no launch)
def _pair():
    p = R.case("one")["pairs"][0]
    return p["coords_src"], p["coords_dst"], p["certainty"], p["depth_src"], p["depth_dst"]


def test_single_pair_argument_checks():
    from sailrecon_amd.utils.io import sample_correspondence_and_depth as f
    cs, cd, c, ds, dd = _pair()
    with pytest.raises(ValueError, match="sample_num"):
        f(cs, cd, c, ds, dd, 0)
    with pytest.raises(ValueError, match="sample_num"):
        f(cs, cd, c, ds, dd, -3)
    with pytest.raises(ValueError, match="mismatched lengths"):
        f(np.zeros((3, 2), np.float32), cd, c, ds, dd, 4)
    with pytest.raises(ValueError, match="mismatched lengths"):
        f(cs, cd, torch.zeros(2), ds, dd, 4)
    with pytest.raises(ValueError, match="end in 2"):
        f(np.zeros((1, 3), np.float32), cd, c, ds, dd, 4)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        f(cs, cd, c, ds[0], dd, 4)
    with pytest.raises(ValueError, match="uniforms"):
        f(cs, cd, c, ds, dd, 4, uniforms=np.zeros(5))


def test_batch_argument_checks():
    from sailrecon_amd.train.data import correspondence_batch as f
    cs, cd, c, ds, dd = _pair()
    corr = dict(coords_src=cs, coords_dst=cd, certainty=c)
    with pytest.raises(ValueError, match="sample_num"):
        f([(0, 1, corr)], [ds, dd], sample_num=0)
    with pytest.raises(IndexError, match="dst_view 2"):
        f([(0, 2, corr)], [ds, dd], sample_num=4)
    with pytest.raises(IndexError, match="src_view -1"):
        f([(-1, 0, corr)], [ds, dd], sample_num=4)
    with pytest.raises(ValueError, match="pair 1.*mismatched lengths"):
        f([(0, 1, corr), (1, 0, dict(corr, certainty=np.zeros(7, np.float32)))], [ds, dd], sample_num=4)
    with pytest.raises(ValueError, match="no pairs"):
        f([], [ds, dd], sample_num=4)
    png = {k: np.zeros((3, 4), np.uint16) for k in ("x_png", "y_png", "conf_png")}
    with pytest.raises(ValueError, match="pair 0"):
        f([(0, 1, dict(png, y_png=np.zeros((4, 3), np.uint16)))], [ds, dd], sample_num=4)
    with pytest.raises(ValueError, match="uint16"):
        f([(0, 1, dict(png, conf_png=np.zeros((3, 4), np.float32)))], [ds, dd], sample_num=4)
    with pytest.raises(ValueError, match="uniforms"):
        f([(0, 1, corr)], [ds, dd], sample_num=4, uniforms=np.zeros((2, 4)))


def test_default_uniforms_draw_from_numpy_global_state():
    """uniforms=None consumes np.random.random_sample((P, K)): the reference's draws, pair after pair."""
    from sailrecon_amd.utils.io import corres_uniforms
    np.random.seed(11)
    u = corres_uniforms(None, 3, 7)
    ref = np.random.RandomState(11).random_sample(3 * 7 + 1)
    assert u.dtype == torch.float64 and np.array_equal(u.numpy().reshape(-1), ref[:-1])
    assert np.random.random_sample() == ref[-1]
