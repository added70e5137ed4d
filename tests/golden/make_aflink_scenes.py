"""Chooses the scenes of tests/test_gpu_aflink.py's end-to-end cases and writes their seeds to aflink_scenes.json.

A scene (tests/aflink_ref.scene) qualifies if, with the calibrated network of `model_seed`, no float64 cost lies within 1e-4 of a
thr_p and the SciPy matching is unchanged under 16 seeded perturbations of +-1e-4 at every thr_p: a device whose costs are within
1e-4 of the float64 ones then links the same tracklets.  Only the seeds are stored; the test rebuilds the scenes.

    python -m tests.golden.make_aflink_scenes
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODEL_SEED, THR_P, WANT = 0, (0.05, 0.5), 4
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "aflink_scenes.json")


def main():
    from tests import aflink_ref
    model = aflink_ref.calibrated(MODEL_SEED)
    seeds, tried = [], 0
    while len(seeds) < WANT:
        if aflink_ref.scene_qualifies(aflink_ref.scene(tried), model, THR_P):
            seeds.append(tried)
        tried += 1
    with open(PATH, "w") as f:
        json.dump({"model_seed": MODEL_SEED, "thr_p": list(THR_P), "margin": 1e-4, "trials": 16, "scenes": seeds}, f, indent=1)
        f.write("\n")
    print(f"{len(seeds)} of {tried} scenes qualify: {seeds}")


if __name__ == "__main__":
    main()
