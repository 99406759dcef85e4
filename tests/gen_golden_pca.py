"""Regenerates tests/golden/pca_fit.npz: small float32 inputs and what sklearn.decomposition.PCA returns for them (fitted on
their float64 copies), with a ratio and with an integer n_components.  tests/test_pca_ref64_cpu.py pins tests/pca_ref64.py to
it on machines without sklearn.

    python tests/gen_golden_pca.py          (needs scikit-learn; the committed file was made with 1.7.2)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_ref64 as R  # noqa: E402

CASES = {           # name -> (F, D, rank, decay, noise, seed, n_components)
    "wide_ratio": (64, 160, 12, 0.7, 0.02, 11, 0.9),
    "wide_int": (64, 160, 12, 0.7, 0.02, 11, 7),
    "tall_ratio": (129, 111, 20, 0.8, 0.01, 12, 0.97),
    "tall_int": (129, 111, 20, 0.8, 0.01, 12, 5),
    "narrow_ratio": (300, 37, 37, 0.85, 0.05, 13, 0.95),
    "narrow_int": (300, 37, 37, 0.85, 0.05, 13, 36),
}


def main():
    import sklearn
    from sklearn.decomposition import PCA
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (F, D, rank, decay, noise, seed, nc) in CASES.items():
        x = R.tracks(F, D, rank, decay, noise, seed)
        p = PCA(n_components=nc, svd_solver="full").fit(x.astype(np.float64))
        stem = name.rsplit("_", 1)[0]
        out[stem + ".x"] = x
        out[name + ".n_components"] = np.array(float(nc))
        out[name + ".mean"] = p.mean_
        out[name + ".components"] = p.components_
        out[name + ".variance"] = p.explained_variance_
        out[name + ".ratio"] = p.explained_variance_ratio_
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_fit.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
