#!/usr/bin/env python
"""Record scikit-learn's PCA of the synthetic code tables of synth_code_tables.py into tests/golden/code_pca_reference.npz (outputs
only; the tests regenerate the tables from their seeds).

Per case: ``sklearn.decomposition.PCA(n_components=2)`` (svd_solver='full', so that the result does not depend on the solver the
'auto' policy picks for a shape) fitted to the table cast to float64, as the reference's draw_figure_epoch fits it
(core/pipelines/voice2pose.py:495-499) -- except for the cast: on the model's float32 table scikit-learn computes in float32, which
costs about 1e-5 absolute on coordinates of magnitude 8.  The float64 fit is the yardstick.  Stored: mean_, components_,
explained_variance_, explained_variance_ratio_, X = transform(table) (every row, or the fixed subsample of the 100000-row case) and
the three leading eigenvalues (the gap check).  Needs scikit-learn >= 1.5 (components signed by their largest entry, svd_flip with
u_based_decision=False); recorded with 1.7.

Usage:  python tests/golden/make_code_pca_reference.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth_code_tables as S  # noqa: E402

OUT = os.path.join(HERE, "code_pca_reference.npz")


def main():
    import sklearn
    from sklearn.decomposition import PCA
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for case in S.CASES:
        t = S.case_table(case)
        x = t.reshape(-1, t.shape[-1]).astype(np.float64)
        pca = PCA(n_components=2, svd_solver="full").fit(x)
        lam = PCA(n_components=3, svd_solver="full").fit(x).explained_variance_
        gaps = S.check_gaps(lam)
        if min(gaps) < S.MIN_GAP:
            raise SystemExit("%s: relative eigenvalue gaps %.4f / %.4f below %.2f -- choose another seed" % ((case,) + gaps + (S.MIN_GAP,)))
        X = pca.transform(x)
        out[case + "/mean"] = pca.mean_
        out[case + "/components"] = pca.components_
        out[case + "/explained_variance"] = pca.explained_variance_
        out[case + "/explained_variance_ratio"] = pca.explained_variance_ratio_
        out[case + "/X"] = X[S.subsample_rows(case, x.shape[0])]
        out[case + "/max_abs_X"] = np.abs(X).max()
        out[case + "/lambda3"] = lam
        print("%-8s %-14s gaps %.4f %.4f  evr %.5f %.5f  max|X| %.3f" % ((case, t.shape) + gaps + tuple(pca.explained_variance_ratio_)
                                                                       + (np.abs(X).max(),)))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
