"""What every plan of a search launch must satisfy (GpuIndex.last_search_plan(), include/hnsw_gpu_diag.h), read off the kernels' use of the
LDS carve (csrc/device_search.h, device_search_generic.h, device_search_wide.h) and off plan_search / plan_geometry (csrc/gpu_search.hip) — not
measured.  Shared by tests/test_search_plan_emu.py (the emulated library), tests/test_gpu_kernel_census.py (the device) and
tests/experiments/search_plan_ab.py; plus the small index both CPU users launch on."""
import numpy as np

BEAM, GENERIC_LDS, GENERIC_HBM, WIDE = 0, 1, 2, 3              # csrc/search_kernels.h SearchForm
TEAM_CTL_BYTES = 160                                           # csrc/device_search.h sizeof(TeamCtl): 8 words + 2 * SLICE_ROWS floats
LDS_PER_CU = 160 * 1024


def round_up(x, m):
    return (x + m - 1) // m * m


def plan_violations(p, ef, max_lds):
    """the conditions `p` (a last_search_plan() dict) breaks, as strings; ef = the beam the launch ran with (the request's, clamped to the
    index size); max_lds = the device's per-block limit of dynamic LDS"""
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)
    team, wpb, wb, lds = bool(p["team"]), p["wpb"], p["wave_bytes"], p["lds"]
    # sizes
    need(wb % 16 == 0, "wave_bytes % 16")
    need(wb <= LDS_PER_CU, "wave_bytes <= 160 KiB")
    need(lds == wpb * wb + (wpb * TEAM_CTL_BYTES if team else 0), "lds == wpb * wave_bytes (+ the team's control blocks)")
    if team:
        need(2 <= wpb <= 8, "team: 2 <= wpb <= 8")
        need(lds <= max_lds, "team: lds within the per-block limit")
        need(p["off_ctl"] == wpb * wb, "team: off_ctl == wpb * wave_bytes")
    else:
        need(lds <= 64 * 1024, "lds <= 64 KiB unless team")
    # order of the regions (the generic form with its sets in HBM counts off_res / off_cand in keys inside the slot's area, not in LDS bytes)
    if p["form"] != GENERIC_HBM:
        need(p["qpad_floats"] * 4 <= p["off_res"] <= p["off_cand"] < p["off_newid"], "qpad_floats * 4 <= off_res <= off_cand < off_newid")
    else:
        need(p["qpad_floats"] * 4 <= p["off_newid"] and (p["off_res"], p["off_cand"]) == (0, ef + 1), "generic in HBM: the sets' key offsets")
    need(p["off_newdist"] == p["off_newid"] + 256, "off_newdist == off_newid + 256")
    need(p["off_newdist"] + 512 <= wb, "off_newdist + 512 <= wave_bytes")
    if p["form"] == BEAM:
        h = p["hcap"]
        need(p["ureg"] in (2, 4, 8, 16) and ef <= 64 * p["ureg"], "beam: ureg")
        if h:
            need(h % 32 == 0 and 512 <= h <= 4096, "beam: hcap % 32, 512 <= hcap <= 4096")
            need(p["off_hash"] + 4 * h <= p["off_newid"], "beam: off_hash + 4 * hcap <= off_newid")
            need(h >= 4 and p["hmagic"] == -((-(1 << 38)) // (h // 4)), "beam: hmagic == ceil(2^38 / (hcap / 4))")
        need(p["off_cand"] + round_up(8 * ef, 16) <= p["off_newid"], "beam: off_cand + round_up(8 * ef, 16) <= off_newid")
    else:
        need(p["ureg"] == 0 and not team, "not beam: no set registers, no team")
    if team:
        need(p["tm_off_ex"] < p["tm_off_miss"] < p["tm_off_lctag"] <= p["tm_off_lcstate"] < p["tm_off_lclinks"] < p["tm_off_dc"], "team: order of the donated region")
        need(p["tm_lcslots"] in (4, 8, 16, 32), "team: tm_lcslots")
        need(p["tm_dccap"] >= 128, "team: tm_dccap >= 128")
        need(p["tm_off_dc"] + 8 * p["tm_dccap"] <= p["off_newid"], "team: tm_off_dc + 8 * tm_dccap <= off_newid")
    need(1 <= p["team_mains"] <= wpb, "1 <= team_mains <= wpb")
    if p["form"] == GENERIC_HBM:
        need(p["set_stride"] == 3 * ef + 2, "generic in HBM: set_stride == 3 * ef + 2")
    elif p["form"] == WIDE:
        P = p["wide_p"]
        need(P >= ef and P & (P - 1) == 0, "wide: wide_p a power of two >= ef")
        need(p["wide_nc"] <= 1024, "wide: wide_nc <= 1024")
        need(p["wide_ch"] > 0 and p["wide_nr"] == -(-ef // p["wide_ch"]), "wide: wide_nr == ceil(ef / wide_ch)")
        need(p["set_stride"] == 3 * P, "wide: set_stride == 3 * wide_p")
    else:
        need(p["set_stride"] == 0, "no HBM sets: set_stride == 0")
    need(p["slots"] == p["blocks"] * wpb and p["blocks"] >= 1, "slots == blocks * wpb")
    return bad


def sparse_index(pg, oracle, dim, m, func, n, linked=40, efc=40, seed=1):
    """An index of n elements of which only the first `linked` form a graph (oracle.PortIndex); the others are isolated zero rows.  A plan
    depends on n (the beam is clamped to it), never on the graph, and a walk over a few dozen rows costs the emulator milliseconds."""
    from pg_embedding_amd.datasets import gmm
    port = oracle.PortIndex(dim, m, efc, 16, func)
    port.add(gmm(linked, dim, k=4, seed=seed))
    meta = pg.make_meta(dim, m, efc, 16, func)
    img = np.zeros(n * int(meta.size_data_per_element), np.uint8)
    raw = np.frombuffer(np.ascontiguousarray(port.raw()), np.uint8)[: linked * int(meta.size_data_per_element)]
    img[: raw.size] = raw
    return pg.GpuIndex.from_flat(meta, img, n, device=0)


class Out:
    """output arrays of one device-pointer call on the emulated library (its device memory is host memory)"""

    def __init__(self, nq, ef, base=False):
        self.lab = np.zeros((nq, ef), np.uint32 if base else np.uint64)
        self.dst = np.zeros((nq, ef), np.float32)
        self.cnt = np.zeros(nq, np.uint32)
        self.st = np.zeros((nq, 2), np.uint32)

    def args(self):
        return self.lab.ctypes.data, self.dst.ctypes.data, self.cnt.ctypes.data, self.st.ctypes.data


def batch_dev(ix, Q, ef, rows=0, caller_order=False, base=False):
    """hnsw_gpu_search_batch_dev / _caller_order_dev / _search_base_dev / _batch_reduced_dev with host arrays: the return code"""
    o = Out(len(Q), ef, base)
    if rows:
        return ix.L.hnsw_gpu_search_batch_reduced_dev(ix._h, rows, Q.ctypes.data, len(Q), ef, *o.args(), None)
    f = ix.L.hnsw_gpu_search_base_dev if base else ix.L.hnsw_gpu_search_batch_caller_order_dev if caller_order else ix.L.hnsw_gpu_search_batch_dev
    return f(ix._h, Q.ctypes.data, len(Q), ef, *o.args(), None)
