"""Records tests/golden/orthotropic_frames.npz from ``orthotropic_ref.update_mp`` (50 digits, fourth-order tensor form): per parameter
set 60 points -- six of every frame class -- with random strains at scale 1e-3.  The metadata stores the largest deviation of the
float64 restatement ``orthotropic_ref.update`` from these values, relative to the field scale (largest |stress| / |tangent entry| of
the parameter set): the GPU bound is max(1e-12, 8 x that).

    python tests/golden/make_orthotropic_frames.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orthotropic_ref as orf  # noqa: E402

POINTS_PER_SET = 60


def deviation(arrays):
    """largest |float64 restatement - fixture| / field scale over all sets: (stress, tangent)"""
    worst = [0.0, 0.0]
    for name, p in orf.PARAMETER_SETS.items():
        eps, R = arrays[f"{name}/eps"], arrays[f"{name}/R"]
        sig, ct = orf.update(eps, p, R)
        for k, (got, want) in enumerate(((sig, arrays[f"{name}/sig"]), (ct, arrays[f"{name}/ct"]))):
            worst[k] = max(worst[k], float(np.abs(got - want).max() / np.abs(want).max()))
    return worst


def main():
    arrays = {}
    for s, (name, p) in enumerate(orf.PARAMETER_SETS.items()):
        labels, R = orf.frames(POINTS_PER_SET, seed=100 + s)
        eps = orf.strains(POINTS_PER_SET, seed=200 + s)
        out = [orf.update_mp(eps[i], p, R[i]) for i in range(POINTS_PER_SET)]
        arrays[f"{name}/eps"], arrays[f"{name}/R"] = eps, R
        arrays[f"{name}/sig"] = np.array([o[0] for o in out])
        arrays[f"{name}/ct"] = np.array([o[1] for o in out])
        arrays[f"{name}/labels"] = labels
    dev = deviation(arrays)
    meta = {"digits": 50, "points_per_set": POINTS_PER_SET, "sets": {k: list(v) for k, v in orf.PARAMETER_SETS.items()},
            "restatement_deviation": {"stress": dev[0], "tangent": dev[1]}}
    np.savez_compressed(os.path.join(HERE, "orthotropic_frames.npz"), meta=json.dumps(meta), **arrays)
    print(json.dumps(meta["restatement_deviation"]))


if __name__ == "__main__":
    main()
