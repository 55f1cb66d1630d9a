"""Writes tests/golden/g23_two_view.npz: the restatement's outputs (tests/two_view_ref.py) on three synthetic pairs,
so that the restatement cannot drift.  Inputs and every output are stored; tests/test_two_view.py compares the drawn
indices, the costs of the stored models and the counts exactly, and the solved models up to sign and rounding.

    python tests/golden/make_golden_two_view.py
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import two_view_ref as T  # noqa: E402

SEEDS, K, H, ITERS, SEED, TAU = (7, 8, 9), 300, 64, 4, 20261021, 2.0


def main():
    src, dst, intr, si, di, ext = T.stack_pairs([T.make_pair(s, K, 0.15, 0.5) for s in SEEDS])
    mask = (np.random.default_rng(1).random((len(SEEDS), K)) < 0.9).astype(np.uint8)
    src[1, 17, 0] = np.nan
    o = T.two_view(src, dst, intr, si, di, mask=mask, n_hyp=H, tau=TAU, iters=ITERS, seed=SEED, ref_extrinsic=ext)
    np.savez_compressed(T.GOLDEN, src=src, dst=dst, intrinsic=intr, src_idx=si, dst_idx=di, ext=ext, mask=mask,
                        n_hyp=H, iters=ITERS, seed=SEED, tau=TAU, **{"out_" + k: v for k, v in o.items()})
    print(T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes; status", o["status"], "pose errors", o["pose_err"].tolist())


if __name__ == "__main__":
    main()
