"""bop_scene._pair_layout and _keep_best, the group layout and the trimming that eval_results and eval_coco share,
against the layout krrn_bop_match_f64 / krrn_coco_match_f64 read and the order they rank by, as bop_match_ref and
coco_ref restate them. Host only."""
import numpy as np

import bop_match_ref as mr
import coco_ref as cr
from pose_estimation_amd import bop, bop_scene, coco

NAN = float("nan")
N_A = [3, 0, 2, 0, 1, 5, 128]                            # ragged, with 0 x n, n x 0 and 0 x 0 groups
N_B = [2, 4, 0, 0, 1, 3, 128]


def test_pair_layout_is_the_layout_the_kernels_read():
    ra, rb, po, P = bop_scene._pair_layout(N_A, N_B)
    assert [n for _, n in ra] == N_A and [n for _, n in rb] == N_B
    assert P == sum(a * b for a, b in zip(N_A, N_B))
    # the rows of each side follow each other group by group; so do the pair blocks, without a gap
    assert [f for f, _ in ra] == np.concatenate([[0], np.cumsum(N_A)[:-1]]).tolist()
    assert [f for f, _ in rb] == np.concatenate([[0], np.cumsum(N_B)[:-1]]).tolist()
    assert po == np.concatenate([[0], np.cumsum(np.multiply(N_A, N_B))[:-1]]).tolist()
    # a pair list written group by group, a-major (eval_results' and eval_coco's loops), read back the way
    # bop_match_ref.match_poses reads err: err[p0 : p0 + ne * ng].reshape(ne, ng)[e, j] is the pair (e0 + e, g0 + j)
    pairs = np.array([(a0 + e, b0 + j) for (a0, na), (b0, nb) in zip(ra, rb) for e in range(na) for j in range(nb)],
                     np.int64).reshape(-1, 2)
    assert len(pairs) == P
    for (a0, na), (b0, nb), p0 in zip(ra, rb, po):
        block = pairs[p0:p0 + na * nb].reshape(na, nb, 2)
        assert (block[:, :, 0] == a0 + np.arange(na)[:, None]).all()
        assert (block[:, :, 1] == b0 + np.arange(nb)[None, :]).all()


def test_pair_layout_of_no_group():
    assert bop_scene._pair_layout([], []) == ([], [], [], 0)


def test_keep_best_cuts_130_tied_and_nan_rows_to_128():
    rng = np.random.default_rng(5)
    scores = rng.integers(0, 4, 130).astype(np.float64) / 4.0      # four distinct values: ties everywhere
    scores[[0, 17, 64, 129]] = NAN                                  # NaN ranks as -inf: last, the lower index first
    scores[[1, 128]] = 0.0                                          # ties with nothing below them but the NaNs
    rows = [{"score": 9.0}] * 7 + [{"score": float(s)} for s in scores]  # the group's rows are not the first ones
    idx = list(range(7, 137))
    kept = bop_scene._keep_best(rows, idx, 128)
    assert len(kept) == 128 and kept == sorted(kept)               # the survivors stay in file order
    assert kept == [idx[i] for i in sorted(mr.order(scores, 128))]  # krrn_bop_match_f64's order
    assert kept == [idx[i] for i in sorted(cr.order(scores)[:128])]  # krrn_coco_match_f64's order
    # what falls out: the two NaN rows with the highest indices
    assert sorted(set(idx) - set(kept)) == [7 + 64, 7 + 129]
    # and the matching order of the survivors is the order of the full group, cut
    sub = [rows[r]["score"] for r in kept]
    assert [kept[i] for i in cr.order(sub)] == [idx[i] for i in cr.order(scores)[:128]]


def test_keep_best_leaves_a_group_within_the_limit_alone():
    rows = [{"score": s} for s in (0.1, NAN, 0.9)]
    for idx in ([], [2], [2, 0, 1]):
        assert bop_scene._keep_best(rows, idx, 3) == idx
    assert bop_scene._keep_best(rows, [0, 1, 2], 2) == [0, 2]
    assert bop_scene._keep_best(rows, [0, 1, 2], 0) == []


def test_one_limit():
    assert bop.MATCH_MAX == coco.MATCH_MAX == mr.MAX == 128
