"""Rows whose distance is NaN, on the SIMT-emulated library (tests/filtered_knn_util.nan_case: 900 x 16, five rows with a NaN coordinate, three
bitmaps, five queries).  Exact filtered k-NN has no threshold, so it returns a NaN row wherever the list has room for it, behind every number;
exact radius search at r = +inf compares d <= r and returns none.  Every form of the filtered call — listed, matrix cores (the filter
replaced by its stand-in, HNSW_GPU_FK_SAMPLE_MIN = 64), automatic with HNSW_GPU_FK_AUTO_SPLIT cutting between the six-row list and the
others — must return the listed form's bytes.  Run as a subprocess by tests/test_filtered_knn_nan_emu.py.  Prints one JSON line: a list of
case reports.

    python tests/emu/run_filtered_knn_nan_case.py <l2 | cosine> [emulated-library]
"""
import json
import sys

import run_filtered_knn_case as R                          # (chooses the library from argv before it imports the package)
import run_filtered_knn_mfma_case as M
import run_range_knn_case as G
import run_filtered_knn_auto_case as A
import numpy as np
import filtered_knn_util as U

NAMES = ("labels", "dists", "idx", "counts")
CUT = 100                                                  # rows: the lists of 900 and 450 rows are loose, the one of six is not


def run(func):
    out, ix = [], None
    for k in (10, 3):
        case = U.nan_case(900, func, k)
        ix = ix or R.mirror(case)
        want = U.nan_expect(case)
        rep = {"case": case["name"], "nbad": 0, "bad": [], "sizes": [w[3] for w in want], "finite": [len(w[0]) for w in want]}

        def note(tag, bad):
            rep["nbad"] += len(bad)
            rep["bad"] += [tag + ": " + str(b) for b in bad[:4]]

        M.knobs(ix.L, True)
        A.split(ix.L, None)
        rc, ref = R.call_dev(ix, case["Q"], k, case["allow"], case["allow_of"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        note("listed", U.nan_check(case, ref, want))                # (NaN rows LAST: the host arithmetic keeps the sign bit of the NaN coordinate clear)
        rep["counts"] = ref["counts"].tolist()
        rep["form_listed"] = ix.last_filtered_knn_form()
        rc, got = M.call_dev(ix, case["Q"], k, case["allow"], case["allow_of"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        rep["form_mfma"] = ix.last_filtered_knn_form()
        note("mfma", U.nan_check(case, got, want) + [("bytes", n) for n in NAMES if got[n].tobytes() != ref[n].tobytes()])
        A.split(ix.L, CUT)
        rc, got = A.fk_auto(ix, case["Q"], k, case["allow"], case["allow_of"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        rep["form_auto"], rep["plan"] = ix.last_filtered_knn_form(), got["plan"].tolist()
        note("auto", U.nan_check(case, got, want) + [("bytes", n) for n in NAMES if got[n].tobytes() != ref[n].tobytes()])
        A.split(ix.L, None)
        # radius search at +inf over the same inputs: the finite rows only
        rad = np.full(case["Q"].shape[0], np.inf, np.float32)
        rep["range_counts"] = {}
        for mode, form, totals in G.MODES:
            rc, got = G.call_dev(ix, case["Q"], rad, k, case["allow"], case["allow_of"], form=form, totals=totals)
            assert rc == 0, ix.L.hnsw_gpu_last_error()
            note("range_" + mode, U.nan_check(case, got, want, within=True))
            rep["range_counts"][mode] = got["counts"].tolist()
        out.append(rep)
    return out


if __name__ == "__main__":
    print(json.dumps(run({"l2": U.L2, "cosine": U.COSINE}[sys.argv[1]])))
