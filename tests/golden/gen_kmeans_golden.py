"""Writes tests/golden/kmeans.npz: scikit-learn's answers for the k-means and clustering-score tests.  Run on the CPU with
scikit-learn 1.7.2 (python tests/golden/gen_kmeans_golden.py); it reads only tests/kmeans_ref.py.  The tests read only the .npz.

Recorded:
  * inputs A (n = 777, e = 33, k = 7) and B (n = 1000, e = 64, k = 200) with an initial set of centres taken from the data, and
    KMeans(init=<array>, n_init=1, algorithm='lloyd', tol=0) on them in float64: labels, centres, inertia, n_iter_;
  * the k-means++ case: input A, seed PP_SEED, n_init = 3 — the rows, labels, n_iter and inertia of kmeans_ref.pp64 + lloyd64
    for the seeds PP_SEED .. PP_SEED + 2 (scikit-learn's greedy k-means++ is another algorithm; nothing of it is recorded);
  * label pairs with normalized_mutual_info_score and homogeneity_completeness_v_measure.
It ASSERTS that the inputs are fit for an exact comparison and fails otherwise: along the whole float64 trajectory of every
case no cluster is ever empty and no point is ambiguous (kmeans_ref.lloyd64(check=True)), scikit-learn's labels are lloyd64's,
and no k-means++ draw comes within n 2^-53 of a prefix-sum boundary after the device's fp32 weight error is taken off
(kmeans_ref.pp64's margin).
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import KMeans
from sklearn.metrics import homogeneity_completeness_v_measure, normalized_mutual_info_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_ref as R  # noqa: E402

PP_SEED = 8


def fit_case(name, n, e, k, noise, seed, init_rows):
    x, _ = R.blobs(n, e, k, noise, seed)
    init = np.ascontiguousarray(x[init_rows])
    ref = R.lloyd64(x, init, check=True)
    assert ref["n_empty_max"] == 0, f"{name}: a cluster went empty"
    assert ref["ambiguous_max"] == 0.0, f"{name}: ambiguous points ({ref['ambiguous_max']})"
    km = KMeans(k, init=init.astype(np.float64), n_init=1, algorithm="lloyd", tol=0).fit(x.astype(np.float64))
    assert np.array_equal(km.labels_, ref["labels"]) and km.n_iter_ == ref["n_iter"], f"{name}: scikit-learn and lloyd64 differ"
    assert abs(km.inertia_ - ref["inertia"]) <= 1e-9 * ref["inertia"]
    print(f"{name}: n_iter {km.n_iter_}, inertia {km.inertia_:.6f}")
    return {f"{name}_x": x, f"{name}_init": init, f"{name}_labels": km.labels_.astype(np.int32),
            f"{name}_centres": km.cluster_centers_.astype(np.float64), f"{name}_inertia": np.float64(km.inertia_),
            f"{name}_n_iter": np.int64(km.n_iter_)}


def pp_case(x, k):
    out = {"pp_seed": np.int64(PP_SEED)}
    n = x.shape[0]
    rows, labels, n_iter, inertia = [], [], [], []
    for r in range(3):
        rr, margin = R.pp64(x, k, PP_SEED + r)
        assert margin > n * 2.0 ** -53, f"k-means++ seed {PP_SEED + r}: a draw sits on a prefix-sum boundary ({margin})"
        assert len(set(rr.tolist())) == k
        ref = R.lloyd64(x, x[rr], check=True)
        assert ref["n_empty_max"] == 0 and ref["ambiguous_max"] == 0.0, f"k-means++ seed {PP_SEED + r}: unfit trajectory"
        rows.append(rr); labels.append(ref["labels"]); n_iter.append(ref["n_iter"]); inertia.append(ref["inertia"])
        print(f"k-means++ seed {PP_SEED + r}: rows {rr.tolist()}, n_iter {ref['n_iter']}, inertia {ref['inertia']:.6f}, margin {margin:.2e}")
    best = np.sort(inertia)
    assert best[1] - best[0] > 1e-4 * best[0], "k-means++: the two best runs tie in inertia"
    out.update(pp_rows=np.asarray(rows, np.int64), pp_labels=np.asarray(labels, np.int32), pp_n_iter=np.asarray(n_iter, np.int64),
               pp_inertia=np.asarray(inertia, np.float64))
    return out


def label_pairs():
    rs = np.random.RandomState(7)
    a = rs.randint(0, 10, 500)
    pairs = {
        "random": (a, rs.randint(0, 10, 500)),
        "random_unequal_counts": (rs.randint(0, 4, 300), rs.randint(0, 17, 300)),
        "random_small": (rs.randint(0, 3, 12), rs.randint(0, 3, 12)),
        "noisy_copy": (a, np.where(rs.rand(500) < 0.8, a, rs.randint(0, 10, 500))),
        "perfect": (a, a.copy()),
        "permuted_ids": (a, rs.permutation(10)[a]),
        "strings": (np.asarray(["cat", "dog", "cat", "eel", "dog", "cat", "eel", "eel"]),
                    np.asarray(["x", "y", "x", "x", "y", "x", "z", "z"])),
        "strings_vs_ints": (np.asarray(["a", "b", "b", "a", "c", "c"]), np.asarray([5, 5, 9, 9, 2, 2])),
        "both_one_cluster": (np.zeros(20, np.int64), np.full(20, 4, np.int64)),
        "true_one_cluster": (np.zeros(30, np.int64), rs.randint(0, 3, 30)),
        "pred_one_cluster": (rs.randint(0, 3, 30), np.zeros(30, np.int64)),
        "every_point_its_own": (rs.randint(0, 5, 40), np.arange(40)),
    }
    out = {"pair_names": np.asarray(list(pairs))}
    for name, (t, p) in pairs.items():
        h, c, _ = homogeneity_completeness_v_measure(t, p)
        out[f"pair_{name}_true"], out[f"pair_{name}_pred"] = t, p
        out[f"pair_{name}_scores"] = np.asarray([normalized_mutual_info_score(t, p), h, c], np.float64)
        assert abs(R.nmi64(t, p) - out[f"pair_{name}_scores"][0]) < 1e-12, name
    return out


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out = {}
    out.update(fit_case("A", 777, 33, 7, 0.8, 11, np.random.RandomState(111).choice(777, 7, replace=False)))
    out.update(fit_case("B", 1000, 64, 200, 0.3, 12, np.arange(200)))
    out.update(pp_case(out["A_x"], 7))
    out.update(label_pairs())
    path = os.path.join(HERE, "kmeans.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
