"""Correspondence / depth sampler on the HIP path (sr_corres_sample through ops.corres_sample,
utils.io.sample_correspondence_and_depth and train.data.correspondence_batch) against the
reference's goldens (tests/golden/make_golden_corres.py) and the fp64 restatement (tests/corres_ref.py).

Per golden case: index equal to the golden's with none excluded (every stored uniform lies >= 2^-22
from every edge of the reference's CDF), both coordinate outputs bit-equal, depths within
max(4 * max|golden - fp64|, 2 fp32 ulps of the case's largest depth) of the fp64 bilinear -- the
bound comes from the golden itself (tests/corres_ref.py depth_bound), like test_loss_gpu's 4 x the
reference's own error.

Measured on MI355X (max |gpu - fp64 bilinear| over both depth outputs; the bound beside it;
test_parity prints them):
  case     error      bound
  grid     6.179e-06  2.472e-05
  chunks   7.620e-06  3.048e-05
  sparse   4.916e-06  1.967e-05
  one      1.602e-07  6.407e-07
  png      4.837e-06  1.935e-05
  multi    9.948e-06  3.979e-05
Indices and coordinates are equal in every case.  The errors are the reference's own (fp32
positions and weights): a quarter of the bound.
"""

import numpy as np
import pytest
import torch

import corres_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _records(name, png=False, only=None):
    c = R.case(name)
    recs = []
    for j, p in enumerate(c["pairs"]):
        if only is not None and j != only:
            continue
        keys = ("x_png", "y_png", "conf_png") if png and "x_png" in p else ("coords_src", "coords_dst", "certainty")
        r = {k: _dev(p[k]) for k in keys}
        r["depth_src"], r["depth_dst"] = _dev(p["depth_src"]), _dev(p["depth_dst"])
        recs.append(r)
    return recs


def _run(name, png=False, only=None):
    from sailrecon_amd import ops
    c = R.case(name)
    u = c["uniforms"] if only is None else c["uniforms"][only:only + 1]
    out = ops.corres_sample(_records(name, png, only), _dev(u), c["min_conf"])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("index", "src_coords", "dst_coords", "src_depth", "dst_depth", "total",
                                                 "n_valid"))


@pytest.mark.parametrize("name", R.CASES)
def test_parity(name):
    c, o = R.case(name), R.oracle(name)
    out = _run(name)
    assert torch.equal(out["index"], torch.from_numpy(c["index"]))
    assert torch.equal(out["src_coords"], torch.from_numpy(c["out_src_coords"]))
    assert torch.equal(out["dst_coords"], torch.from_numpy(c["out_dst_coords"]))
    err = 0.0
    for j, (_, _, _, sd, dd) in enumerate(o):
        err = max(err, np.abs(out["src_depth"][j].numpy() - sd).max(), np.abs(out["dst_depth"][j].numpy() - dd).max())
    bound = R.depth_bound(name)
    print(f"corres {name}: depth max|gpu - fp64| {err:.3e}  bound {bound:.3e}")
    assert err <= bound
    for j, p in enumerate(c["pairs"]):
        w = R.weights(p["certainty"], c["min_conf"])
        assert int(out["n_valid"][j]) == int((p["certainty"] > np.float32(c["min_conf"])).sum())
        assert abs(float(out["total"][j]) - w.sum()) <= 1e-12 * w.sum()


def test_png_form_bit_identical_to_array_form():
    assert _same(_run("png", png=True), _run("png"))
    assert _same(_run("multi", png=True), _run("multi"))  # mixed formats in one table


def test_batch_bit_identical_to_single_pair_calls():
    whole = _run("multi")
    for j in range(5):
        one = _run("multi", only=j)
        for k in ("index", "src_coords", "dst_coords", "src_depth", "dst_depth", "total", "n_valid"):
            assert torch.equal(one[k][0], whole[k][j]), (j, k)


def test_run_to_run_and_workspace_reuse():
    a, b = _run("chunks"), _run("chunks")
    assert _same(a, b)
    one = _run("one")          # the workspace of the larger call, reused
    assert _same(_run("chunks"), a)
    from sailrecon_amd import ops
    ops._CORRES_WS.clear()
    one2 = _run("one")         # a fresh, small workspace, then grown
    assert _same(one, one2)
    assert _same(_run("chunks"), a) and _same(_run("one"), one)


@pytest.mark.parametrize("name", ["grid", "multi"])
def test_default_uniforms_follow_numpy_global_state(name):
    from sailrecon_amd.train.data import correspondence_batch
    from sailrecon_amd.utils.io import sample_correspondence_and_depth
    c = R.case(name)
    P, K = c["uniforms"].shape
    np.random.seed(c["seed"])
    if name == "grid":
        p = c["pairs"][0]
        res = sample_correspondence_and_depth(p["coords_src"], torch.from_numpy(p["coords_dst"]), p["certainty"],
                                              p["depth_src"], p["depth_dst"], K, c["min_conf"])
        got = dict(zip(("src_coords", "dst_coords", "src_depth", "dst_depth"), (t[None] for t in res)))
    else:
        pairs = [(s, t, {k: p[k] for k in (("x_png", "y_png", "conf_png") if "x_png" in p else
                                            ("coords_src", "coords_dst", "certainty"))})
                 for (s, t), p in zip(c["views"], c["pairs"])]
        got = correspondence_batch(pairs, c["depths"], sample_num=K, min_corres_conf=c["min_conf"], device=DEV)
        assert got["src_idx"].dtype == torch.long and got["src_idx"].tolist() == [s for s, _ in c["views"]]
        assert got["dst_idx"].tolist() == [t for _, t in c["views"]]
    assert np.random.random_sample() == np.random.RandomState(c["seed"]).random_sample(P * K + 1)[-1]
    want = _run(name)
    for k in ("src_coords", "dst_coords", "src_depth", "dst_depth"):
        assert got[k].is_cuda and got[k].dtype == torch.float32
        assert torch.equal(got[k].cpu(), want[k]), k
    assert torch.equal(got["src_coords"].cpu(), torch.from_numpy(c["out_src_coords"]))
    assert torch.equal(got["dst_coords"].cpu(), torch.from_numpy(c["out_dst_coords"]))


def test_no_eligible_correspondence_raises_naming_the_pair():
    from sailrecon_amd import ops
    from sailrecon_amd.train.data import correspondence_batch
    c = R.case("multi")
    recs = _records("multi")
    with pytest.raises(ValueError, match=r"Pair 3: no correspondence points meet the minimum confidence threshold 0\.75"):
        ops.corres_sample(recs, _dev(c["uniforms"]), 0.75)  # pair 3 is the single 0.7 entry
    out = ops.corres_sample(recs, _dev(c["uniforms"]), 0.75, check=False)
    torch.cuda.synchronize()
    assert float(out["total"][3]) == 0.0 and int(out["n_valid"][3]) == 0
    for k in ("src_coords", "dst_coords", "src_depth", "dst_depth", "index"):
        assert not out[k][3].any(), k
    p = c["pairs"][3]
    with pytest.raises(ValueError, match="Pair 0.*threshold 0.9"):
        correspondence_batch([(0, 1, {k: p[k] for k in ("coords_src", "coords_dst", "certainty")})], c["depths"],
                             sample_num=4, min_corres_conf=0.9, device=DEV)


def test_bad_tensors_rejected_before_any_launch():
    from sailrecon_amd import ops
    c = R.case("grid")
    good = _records("grid")[0]
    u = _dev(c["uniforms"])
    before = ops.last_kernel()
    bad = [dict(good, certainty=good["certainty"].cpu()),                                  # host tensor
           dict(good, certainty=good["certainty"].double()),                               # wrong dtype
           dict(good, coords_dst=good["coords_dst"].half()),
           dict(good, depth_src=good["depth_src"].t()),                                    # non-contiguous
           dict(good, coords_src=torch.cat([good["coords_src"]] * 2, 1)[:, :2]),
           dict(good, coords_src=good["coords_src"][:-1]),                                 # mismatched lengths
           dict(good, depth_dst=good["depth_dst"][0])]                                     # not a map
    for b in bad:
        with pytest.raises(ValueError):
            ops.corres_sample([b], u, 0.1)
    with pytest.raises(ValueError):
        ops.corres_sample([good], u.float(), 0.1)
    with pytest.raises(ValueError):
        ops.corres_sample([good], u.cpu(), 0.1)
    with pytest.raises(ValueError):
        ops.corres_sample([good, good], u, 0.1)
    assert ops.last_kernel() == before  # nothing was launched


def test_loss_hand_off_device_resident_batch():
    """compute_loss on the device-resident dict from correspondence_batch equals, bit for bit, the
    loss on CPU copies of the same arrays."""
    from sailrecon_amd.train.data import correspondence_batch, synthetic_batch
    from sailrecon_amd.train.loss import CDFLossIndexPytorch, compute_loss
    c = R.case("multi")
    pairs = [(s, t, {k: p[k] for k in ("coords_src", "coords_dst", "certainty")})
             for (s, t), p in zip(c["views"], c["pairs"])]
    cb = correspondence_batch(pairs, c["depths"], sample_num=c["K"], min_corres_conf=c["min_conf"],
                              uniforms=c["uniforms"], device=DEV)
    batch = synthetic_batch(3, n_points=c["K"], size=56, seed=3)
    batch.update(cb)
    enc = torch.tensor([[0.1, -0.2, 0.3, 0.05, -0.1, 0.02, 1.0, 1.0, 1.1],
                        [-0.3, 0.1, 0.2, -0.04, 0.08, 0.1, 0.9, 0.95, 1.05],
                        [0.2, 0.2, -0.1, 0.1, 0.02, -0.06, 1.1, 1.2, 0.9]], device=DEV)
    cdf = CDFLossIndexPytorch(0.0, 15.0, 250, cb["src_idx"].cpu(), cb["dst_idx"].cpu(), gradient_smooth=0.05)
    on_dev = compute_loss(enc, batch, DEV, cdf, image_hw=(56, 56))
    host = dict(batch, **{k: v.cpu() for k, v in cb.items()})
    on_host = compute_loss(enc, host, DEV, cdf, image_hw=(56, 56))
    assert torch.isfinite(on_dev["loss"]).all()
    assert torch.equal(on_dev["loss"], on_host["loss"]) and torch.equal(on_dev["d_pose_enc"], on_host["d_pose_enc"])
