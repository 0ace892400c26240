"""The random cases of tests/random_cases.py, checked on the CPU for every seed tests/test_random_analytics_gpu.py runs: the draw is
reproducible; prune_ref.edges' threshold guard trips on no case; the references agree with each other where their definitions
overlap, and their seven ``unpack`` copies agree on the one selection of the one buffer every case holds; the FP64 bounds of the
real-valued cases tell a right entry from a wrong one; and, over the whole seed set, every edge, kind and flag the generator is
meant to reach was reached."""
import numpy as np
import pytest

import gapply_ref as AR
import gram_ref as GR
import matrix_ref as MX
import pack_ref as PK
import pair_ref as PR
import random_cases as RC
import score_ref as SC
import spair_ref as SP
import vsum_ref as VS


def same(a, b) -> bool:
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[key], b[key]) for key in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_draw_is_reproducible(seed):
    again = [RC.draw_case(rng, i) for rng in [np.random.default_rng(RC.SEED_BASE + seed)] for i in range(RC.CASES_PER_SEED)]
    assert same(RC.cases(seed), again)


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_references_agree_on_every_case(seed):
    """``expected`` runs on every case (prune_ref.edges raises ThresholdTooClose on none: a trip is answered by another SEED_BASE, never
    by catching it), and on its results and the case's one code matrix:
      per-variant counts = row and column marginals of the pair tables = variant sums of all-ones values;
      per-sample counts = the diagonal of the sample-pair tables;
      sample_gram of one-hot tables = the [x][x] entries of the sample-pair tables;
      scores with weights 1 and miss 0 = c1 + 2 c2;
      gram_apply's exact Y = the exact Gram rows times q;
      every reference module's own unpack of the selected records = the code matrix."""
    for c in RC.cases(seed):
        tag = f"seed={seed} case={c['index']} {RC.describe(c)}"
        e = RC.expected(c)
        codes, v, k, n, kept = c["codes"], c["v"], c["k"], c["n"], c["kept"]
        gc, sc = e["genotype_counts"], e["sample_counts"]
        assert gc.sum() == sc.sum() == v * k and (gc.sum(axis=1) == k).all() and (sc.sum(axis=1) == v).all(), tag
        # the seven unpack copies on the bytes the calls read
        recs = c["recs_sel"]
        if n % 4:
            assert (recs[:, -1] >> (2 * (n % 4))).all(), f"{tag}: a row's pad bits are clean"
        pick = slice(None) if kept is None else kept
        unpacked = [PR.unpack(recs, n, kept), SP.unpack(recs, n, kept), GR.unpack(recs, n, kept), AR.unpack(recs, n, kept), MX.codes(recs, n, kept),
                    SC.unpack_codes(recs, n)[:, pick], VS.unpack_codes(recs, n)[:, pick], PK.unpack(recs, n)[:, pick],
                    PK.unpack(PK.pack(recs, n, kept), k)]
        for i, u in enumerate(unpacked):
            assert np.array_equal(u, codes), f"{tag}: unpack {i} disagrees with the code matrix"
        # pair tables' marginals
        t = e["pair_tables"]
        for i, d in PR.pair_list(v, c["n_left"], c["w"]):
            assert np.array_equal(t[i, d - 1].sum(axis=1), gc[i]) and np.array_equal(t[i, d - 1].sum(axis=0), gc[i + d]), f"{tag}: pair ({i}, {i + d})"
        ones, _ = VS.vsum_from_codes(codes, np.ones((k, 1)))
        assert np.array_equal(ones[:, 0, :], gc.astype(np.float64)), tag
        # sample-pair tables: the diagonal, and the Gram matrix of one-hot tables
        a, b = c["spair_a"], c["spair_b"]
        diag = SP.ranges(codes, a, a)
        for i in range(a[1]):
            assert np.array_equal(np.diag(diag[i, i]), sc[a[0] + i]) and diag[i, i].sum() == v, f"{tag}: rank {a[0] + i}"
        for x in range(4):
            onehot = np.zeros((v, 4))
            onehot[:, x] = 1.0
            assert np.array_equal(GR.gram_ref(RC.cols(codes, a), onehot, RC.cols(codes, b)), e["sample_pair_stats"][:, :, x, x].astype(np.float64)), f"{tag}: code {x}"
        s, _ = SC.score_from_codes(codes, np.ones(v, dtype=np.float32))
        assert np.array_equal(s[:, 0], (sc[:, 1] + 2 * sc[:, 2]).astype(np.float64)), tag
        # Y = (Z^T Z) q on the rows of the case's Gram range, in integers
        rng = np.random.default_rng(c["chain_seed"])
        ti, qi = rng.integers(-8, 9, size=(v, 4)).astype(np.float64), rng.integers(-4, 5, size=(k, 3)).astype(np.float64)
        _, y = AR.apply_int(codes, ti, qi)
        ga = c["gram_a"]
        gram_rows = GR.gram_ref(RC.cols(codes, ga), ti, codes)
        assert np.array_equal(y[ga[0]: ga[0] + ga[1]].astype(np.float64), gram_rows @ qi), tag
        if c["fp"] == "int":
            assert np.array_equal(e["gram_apply_y"][ga[0]: ga[0] + ga[1]], GR.gram_ref(RC.cols(codes, ga), c["tables"], codes) @ c["q"]), tag
            assert np.array_equal(e["sample_gram"], GR.gram_fsum(RC.cols(codes, ga), c["tables"], RC.cols(codes, c["gram_b"]))), tag
        else:
            # the bounds tell a right entry from a wrong one: |want| > 100 x bound on more than 0.9 of the sums that have a term
            # (test_gram_apply_gpu.py asserts the same of its own inputs)
            live = RC.nonempty(c, e)
            bounds = {"sample_scores": e["sample_scores_bound"], "variant_sums": e["variant_sums_bound"][None, :, None],
                      "sample_gram": 1.01 * (v + 2) * 2.0 ** -53 * e["sample_gram_abs"],
                      "gram_apply_p": e["gram_apply_p_bound"], "gram_apply_y": e["gram_apply_y_bound"]}
            for name, bound in bounds.items():
                far = (np.abs(e[name]) > 100 * bound)[live[name]]
                assert far.size == 0 or far.mean() > 0.9, f"{tag}: {name}: the bound does not tell a right entry from a wrong one ({far.mean():.3f})"


def test_coverage_census():
    """Over the whole seed set: every N edge and its two neighbours, every record-size edge of the join plan, every keep kind with
    sample 0 and sample N - 1 kept and not, every layout, every W, C, dtype and priority kind, both matrix orders, both FP kinds,
    accumulate on and off in every family that has the flag, every n_left choice, ranges that end at K and a != b, V = 1, and parse
    and join both taken and refused."""
    all_cases = [RC.draw_case(rng, i) for seed in RC.SEEDS for rng in [np.random.default_rng(RC.SEED_BASE + seed)] for i in range(RC.CASES_PER_SEED)]
    seen = lambda key: {c[key] for c in all_cases}
    assert len(RC.SEEDS) >= 30
    assert set(RC.EDGE_NS) <= seen("n"), sorted(set(RC.EDGE_NS) - seen("n"))
    assert set(RC.EDGE_RECORD_SIZES) <= seen("r"), sorted(set(RC.EDGE_RECORD_SIZES) - seen("r"))
    assert {1, 2, 3, 4, 5} <= seen("n") and max(seen("n")) > 8192
    assert seen("keep_kind") == set(RC.KEEP_KINDS) and seen("layout") == set(RC.LAYOUTS)
    for kind in RC.KEEP_KINDS[1:]:
        ends = {(int(c["kept"][0]) == 0, int(c["kept"][-1]) == c["n"] - 1) for c in all_cases if c["keep_kind"] == kind and c["n"] > 8}
        assert ends == {(False, False), (False, True), (True, False), (True, True)}, kind
    assert seen("w") == set(RC.W_LIST) and seen("c") == set(RC.C_LIST) and seen("v") == set(RC.V_LIST)
    assert seen("sample_major") == {False, True} and seen("dtype") == set(RC.DTYPES)
    assert seen("priority_kind") == set(RC.PRIORITY_KINDS) and seen("fp") == {"int", "real"} and seen("all_kept") == {False, True}
    assert {(f, on) for c in all_cases for f, on in c["accumulate"].items()} == {(f, on) for f in RC.ACC_FAMILIES for on in (False, True)}
    assert {(c["n_left"] == c["v"], c["n_left"] == 0) for c in all_cases if c["v"] > 1} == {(True, False), (False, False), (False, True)}
    for a, b in (("spair_a", "spair_b"), ("gram_a", "gram_b")):
        assert any(c[a][0] + c[a][1] == c["k"] and c[a][0] > 0 for c in all_cases) and any(c[b][0] + c[b][1] == c["k"] and c[b][0] > 0 for c in all_cases)
        assert any(c[a] != c[b] for c in all_cases) and any(c[a] == c[b] for c in all_cases)
        assert any(c[a][1] == RC.MAX_RANKS for c in all_cases)
    assert any(c["layout"] == "gathered" and len(set(c["rows"]["variant_idx"].tolist())) < c["v"] for c in all_cases)
    assert any(c["layout"] == "at" and len({int(o) & 1 for o in c["rows"]["record_off"]}) == 2 for c in all_cases)
    assert any(c["code_map"] is None for c in all_cases) and any(c["code_map"] == PK.BED_MAP for c in all_cases)
    assert any(c["fp"] == "real" and c["k"] > 1000 for c in all_cases)
