#!/usr/bin/env python3
"""Record sklearn's own distances for the cases of tests/knn_ref64.py with the reference's arguments (models/gaussians/basics.py:
208-224: NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean"), first column dropped, cast to float32) into
tests/golden/knn/<case>.npz, one array "k<k>" per k of knn_ref64.GOLDEN_KS.  Needs sklearn (recorded with 1.7.2); CPU only.

    python scripts/gen_golden_knn.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import knn_ref64 as R  # noqa: E402


def k_nearest_distances(x, k):
    from sklearn.neighbors import NearestNeighbors
    model = NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean").fit(x)
    distances, _ = model.kneighbors(x)
    return distances[:, 1:].astype(np.float32)


def main():
    import sklearn
    os.makedirs(R.GOLDEN, exist_ok=True)
    total = 0
    for name, ks in R.GOLDEN_KS.items():
        path = os.path.join(R.GOLDEN, f"{name}.npz")
        np.savez_compressed(path, **{f"k{k}": k_nearest_distances(np.array(R.points(name)), k) for k in ks})
        total += os.path.getsize(path)
        print(f"{name}: N = {len(R.points(name))}, k = {ks}, {os.path.getsize(path)} bytes")
    print(f"sklearn {sklearn.__version__}: {total} bytes in all")


if __name__ == "__main__":
    main()
