"""Child process of tests/test_gpu_classifier.py for path B (LITEPI_CLS_LAYERWISE=1, read once per process by
classifier.cpp, so it cannot be switched inside pytest).  Not a test module.

    python tests/cls_layerwise_child.py JOBS.pkl OUT.npz

JOBS.pkl: {"rois": [...], "jobs": [job, ...]} (classifier_pool.run_job's job dicts).  OUT.npz: per job j and call n,
j{j}_ids{n}, j{j}_probs{n}, j{j}_names (kernel names of the first call) and j{j}_error (LitepiError text, '' if none)."""
import os
import pickle
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_ROOT, "tests"), os.path.join(_ROOT, "yolo-litepi_amd"), _ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import classifier_pool as CP  # noqa: E402


def main(jobs_path: str, out_path: str) -> int:
    with open(jobs_path, "rb") as f:
        spec = pickle.load(f)
    out = {}
    for j, job in enumerate(spec["jobs"]):
        res = CP.run_job(job, spec["rois"])
        for n, (ids, probs) in enumerate(zip(res["ids"], res["probs"])):
            out[f"j{j}_ids{n}"] = ids
            out[f"j{j}_probs{n}"] = probs
        out[f"j{j}_names"] = np.array(res["names"], dtype=str)
        out[f"j{j}_error"] = np.array(res["error"])
    np.savez(out_path, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
