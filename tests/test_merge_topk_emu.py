"""The top-k merge of a row-sharded search (topk_merge_kernel, csrc/gpu_sharded.hip) on the SIMT-emulated library: the product's own
kernel source executed on the CPU, compared bit for bit (labels, distance bits, counts, every query) with the numpy reference of
tests/merge_util.py on lists that no search produces — short and empty lists, heavy ties, negative distances, -0.0 / +0.0 / +inf
under real labels, the same (distance, label) in several lists and straddling position ef - 1, 48-bit labels — over
nlists x ef x nq in full, through hnsw_gpu_merge_topk_dev and through hnsw_gpu_merge_topk_strided_dev with unequal strides and
poisoned gaps.  The same comparison fails for four deliberately broken kernels, each by name (the inputs have teeth).
The emulator runs the lanes of a wave in turn: the device tier (tests/test_gpu_merge_topk.py) repeats the comparison on the GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402
import merge_util as M                                     # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_merge_case.py")


def run_case(case, lib, timeout=900):
    r = subprocess.run([sys.executable, RUN, case, lib], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def test_the_generators_keep_the_input_contract_and_reach_the_edges():
    """the inputs themselves: sorted, padded at the tail only, no NaN; and the edges the families exist for are there"""
    both = set()
    for fam in M.FAMILIES:
        for nl, nq, ef, seed in ((1, 1, 1, 0), (1, 1, 1, 1), (2, 1, 7, 2), (2, 1, 7, 3), (3, 9, 64, 4), (17, 3, 100, 5)):
            labels, dists = M.make_lists(fam, nl, nq, ef, seed)
            assert labels.shape == dists.shape == (nl, nq, ef) and labels.dtype == M.np.uint64 and dists.dtype == M.np.float32
            M.check_contract(labels, dists)
            real = (labels != M.NO_LABEL)
            if fam == "short":
                per_query = real.any(axis=2).sum(axis=0)
                if nq > 1:
                    assert (per_query == 0).any() and (per_query == 1).any()
                elif nl > 1:
                    both.add(int(per_query[0]))
            if fam == "specials" and ef >= 64:
                assert (M.np.isinf(dists) & real).any() and (dists.view(M.np.uint32) == 0x80000000).any()
            if fam == "tid":
                assert int(labels[real].max()) >> 47 == 1
            if fam == "overlap":
                within, across = M.duplicate_keys(labels, dists)
                assert within[2:].all() or ef == 1                        # every query after the first two: a key twice inside one list ...
                assert across[2:].all() or nl == 1                        # ... and a key in two lists;
                straddle = M.straddles(labels, dists)                     # the first two hold the pair across position ef - 1
                assert (straddle[:2].all() and M.reference_merge(labels, dists, ef)[2][0] == ef) or nl == 1
            else:
                assert not M.straddles(labels, dists).any() or fam in ("ties", "specials")
    assert both == {0, 1}                                                 # (one-query batches: every list empty, and exactly one list)
    d = M.np.array([-M.np.inf, -1.0, -1e-3, -0.0, 0.0, 1e-3, 1.0, M.np.inf], M.np.float32)
    assert (M.np.diff(M.dist_order(d).astype(M.np.int64)) > 0).all()


def test_the_reference_merges_a_case_worked_by_hand():
    """ef 3, two lists: a padded tail, a key in both lists, -0.0 before +0.0, +inf under a real label"""
    np, N, inf = M.np, M.NO_LABEL, M.np.inf
    labels = np.array([[[5, 9, N]], [[4, 5, 6]]], np.uint64)
    dists = np.array([[[0.0, 2.0, inf]], [[-0.0, 0.0, inf]]], np.float32)
    l, d, c = M.reference_merge(labels, dists, 3)
    assert l.tolist() == [[4, 5, 5]] and d.view(np.uint32).tolist() == [[0x80000000, 0, 0]] and c.tolist() == [3]
    l, d, c = M.reference_merge(labels[:1], dists[:1], 3)
    assert l.tolist() == [[5, 9, int(N)]] and d.tolist() == [[0.0, 2.0, inf]] and c.tolist() == [2]


def test_the_packed_key_form_of_the_reference_equals_its_statement():
    """reference_merge sorts one packed uint64 key where the labels allow it (the device tier's large cases); the statement is the
    np.lexsort over (distance order, label, list): the same bits for every family and shape that the packed form accepts"""
    compared = 0
    for fam, nl, nq, ef, seed in M.emu_grid():
        if fam != "tid" and nl * nq * ef <= 60000:
            labels, dists = M.make_lists(fam, nl, nq, ef, seed)
            assert not M.mismatches(M.reference_merge(labels, dists, ef, packed=True), M.reference_merge(labels, dists, ef, packed=False)).any(), (fam, nl, nq, ef)
            compared += 1
    assert compared > 1000
    labels, dists = M.make_lists("tid", 3, 3, 7, 1)
    with pytest.raises(AssertionError):
        M.reference_merge(labels, dists, 7, packed=True)                  # 48-bit labels: the statement only


def test_merge_equals_the_reference_on_the_whole_grid(emu_lib):
    res = run_case("grid", emu_lib)
    cases = 2 * len(M.emu_grid())                                          # both entry points
    assert sum(f["cases"] for f in res["families"].values()) == cases == 2 * 7 * 6 * 10 * 3
    assert res["comparisons"] == 2 * sum(c[2] for c in M.emu_grid())
    assert res["wrong"] == 0, res["first_wrong"]
    seen = res["seen"]
    assert seen["every_list_empty"] > 0 and seen["one_list_only"] > 0 and seen["short_output"] > 0, seen
    assert seen["straddle"] > 0 and seen["key_twice_in_a_list"] > 0 and seen["key_in_two_lists"] > 0, seen
    print(f"merge on the emulator: {res['comparisons']} (case, query) comparisons in {cases} cases, {res['seconds']} s")


TIE_BREAK = " || (od == d && ol == lab && m < l)"
BROKEN = {
    "a_tie_break_removed": (TIE_BREAK, ""),
    "b_padding_counted_as_below": ("const bool below = (ol != ~0ull) && (", "const bool below = (ol == ~0ull) || ("),
    "c_rank_seeded_with_i_plus_1": ("uint32_t rank = i;", "uint32_t rank = i + 1;"),
    "d_tail_padding_from_0": ("for (uint32_t i = kept + lane; i < ef; i += 64)", "for (uint32_t i = lane; i < ef; i += 64)"),
}


@pytest.mark.parametrize("variant", sorted(BROKEN))
def test_merge_comparison_catches_a_broken_kernel(variant):
    """teeth: the same comparison on gpu_sharded.hip with one deliberate mistake in topk_merge_kernel reports differences"""
    old, new = BROKEN[variant]

    def edit(name, txt):
        if name == "gpu_sharded.hip":
            assert txt.count(old) == 1, (variant, txt.count(old))
            txt = txt.replace(old, new)
        return txt
    res = run_case("quick", build_emu.build_tree(tag="merge_" + variant[0], edit=edit))
    assert res["wrong"] > 0, f"variant {variant} is not caught"
    caught = sorted(f for f, r in res["families"].items() if r["wrong"])
    print(f"variant {variant}: caught, {res['wrong']} of {res['comparisons']} comparisons differ, in families {caught}")
    if variant.startswith("a_"):
        assert caught == ["overlap"], caught                              # equal keys across lists exist in that family only
    if variant.startswith("b_"):
        assert "short" in caught, caught
