"""The launches of this tree and of its parent commit, compared line for line on the CPU (SIMT emulator, tests/emu/build_emu.py).

    python tests/experiments/search_plan_ab.py [--parent-rev HEAD^] [--shards 4] [--out profiles/search_plan_ab.txt]

Two emulator libraries are built: one from `git archive <parent-rev> pg_embedding_amd/csrc` (unpacked under tests/_build/), one from this
tree.  build_tree's `edit` hook puts ONE statement in front of the search kernel's hipLaunchKernelGGL in gpu_search.hip of each: it appends
a line to the file $SEARCH_PLAN_AB_LOG with every non-pointer field of SearchArgs by name, every pointer field as 0 / 1 (null / not),
blocks, threads per block, dynamic LDS bytes and the kernel's name.  The statement is the same in both trees except for the names of the
locals it reads (the parent: blocks, wpb, lds, w->kname; this tree: the SearchPlan p).  A worker process per library and shard drives
the same sweep (knobs through hnsw_gpu_config_set, indexes of 40 linked rows among n isolated ones, so that no beam is clamped and a walk
costs milliseconds); it writes a CASE line before every call and an RC line with the error text after every refused one.  The two logs
must be identical.  On this tree the worker also checks, after every launch of the mirror's own workspace, that last_search_plan() and
last_search_kernel() say what the logged line says.
"""
import argparse
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

NONPTR = ("n dim stride nchunks kiters maxM lstride entry q_stride nq ef ccap pops_cap evals_cap vis_words logcap qpad_floats off_res off_cand "
          "off_newid off_newdist wave_bytes off_hash hcap hmax hmagic out_stride set_stride wide_p wide_ch wide_nr wide_nc mode team_mains off_ctl "
          "tm_off_ex tm_off_miss tm_off_lctag tm_off_lcstate tm_off_lclinks tm_lcslots tm_off_dc tm_dccap tm_spec abort_mask stream_ring stream_light "
          "rstride4 nblk xcd_log2c").split()
PTR = ("vec links labels queries out_labels out_idx out_dists out_counts out_stats out_pops out_evals out_times done vis vlog ticket set_scratch "
       "abort_word health team_dbg stream_host stream_dev rows16 perm").split()
LAUNCH = "\thipLaunchKernelGGL(kern, "

DIMS = (4, 72, 128, 130, 256, 260, 320, 324, 512, 520, 768, 1000, 2000)
EFS = (1, 64, 65, 128, 129, 256, 257, 400, 512, 513, 1000, 2048, 2049, 5000)
KNOB_EFS = (1, 64, 65, 129, 257, 400, 513, 2049)
MS = (4, 12, 48)
N_BIG = 5120                                                    # >= the widest beam of the sweep
ALL_KNOBS = ("TEAM", "NARROW5", "LEAN", "BEAM16", "BEAM", "FORCE_LDS_HEAPS", "LDS_SET_MIN_WAVES", "WIDE_EF_MIN", "REF_ORDER", "TEAM_WPB", "TEAM_SPEC",
             "HASH_ENTRIES", "NARROW_WPB", "BLOCKS_PER_CU", "MAX_BLOCKS", "LOCALITY_MIN_NQ", "TEAM_MAX_NQ")
KNOB_SETS = ([{"TEAM": 0}, {"TEAM": 1}, {"NARROW5": 0}, {"LEAN": 0}, {"BEAM16": 1}, {"BEAM": 0}, {"FORCE_LDS_HEAPS": 1}, {"LDS_SET_MIN_WAVES": 1000},
              {"WIDE_EF_MIN": 0}, {"REF_ORDER": 1}]
             # the pairs of tests/kernel_census.py
             + [{"TEAM": 0, "BEAM16": 1}, {"TEAM": 1, "BEAM16": 1}, {"TEAM": 0, "NARROW5": 0}, {"TEAM": 0, "LEAN": 0}, {"FORCE_LDS_HEAPS": 1, "LDS_SET_MIN_WAVES": 1000}]
             + [{"TEAM": 1, "TEAM_WPB": 2}, {"TEAM": 1, "TEAM_WPB": 3}, {"TEAM": 1, "TEAM_SPEC": 0}, {"HASH_ENTRIES": 512}, {"HASH_ENTRIES": 1024},
                {"TEAM": 1, "TEAM_WPB": 2, "HASH_ENTRIES": 512}, {"TEAM": 0, "NARROW_WPB": 1}, {"BLOCKS_PER_CU": 1}, {"MAX_BLOCKS": 1}, {"TEAM": 1, "MAX_BLOCKS": 1}])


def logging_edit(blocks, threads, lds, name_stmt):
    fmt = " ".join(f"{f}=%llu" for f in NONPTR) + " | " + " ".join(f"{f}=%d" for f in PTR) + " | blocks=%llu threads=%llu lds=%llu kernel=%s\\n"
    args = ", ".join(f"(unsigned long long) a.{f}" for f in NONPTR) + ", " + ", ".join(f"(int) (a.{f} != nullptr)" for f in PTR)
    stmt = ("\t{ const char *abf_ = getenv(\"SEARCH_PLAN_AB_LOG\"); FILE *abo_ = abf_ ? fopen(abf_, \"a\") : nullptr; if (abo_) { " + name_stmt +
            f" fprintf(abo_, \"{fmt}\", {args}, (unsigned long long) ({blocks}), (unsigned long long) ({threads}), (unsigned long long) ({lds}), abn_); fclose(abo_); }} }}\n")

    def edit(f, txt):
        if f == "gpu_search.hip":
            assert txt.count(LAUNCH) == 1
            txt = txt.replace(LAUNCH, stmt + LAUNCH)
        return txt
    return edit


PARENT_EDIT = logging_edit("blocks", "wpb * 64", "lds", "const char *abn_ = w->kname;")
THIS_EDIT = logging_edit("p.blocks", "p.wpb * 64", "p.lds", "char abn_[128]; search_kernel_name(p, abn_, sizeof(abn_));")


# ---------------------------------------------------------------------------------------------------------------------- worker
def worker(log, shard, nshards):
    os.environ["SEARCH_PLAN_AB_LOG"] = log
    os.environ.pop("PGEMB_ENV_SYNC", None)
    import numpy as np
    import pg_embedding_amd as pg
    import oracle
    import search_plan_util as sp
    from pg_embedding_amd.datasets import gmm
    L = pg._lib.gpu_lib()
    has_plan = hasattr(L, "hnsw_gpu_last_search_plan")
    stat = {"cases": 0, "plan_checked": 0, "plan_mismatch": []}

    def say(line):
        with open(log, "a") as f:
            f.write(line + "\n")

    def knobs(ks):
        for k in ALL_KNOBS:
            pg.config_set("HNSW_GPU_" + k, ks.get(k))

    def case(name, call, ix=None):
        """one call: CASE line, the launch lines the library writes, an RC line when it is refused; on this tree the stored plan against the last line"""
        stat["cases"] += 1
        say("CASE " + name)
        rc = call()
        if rc:
            say(f"RC {rc} {L.hnsw_gpu_last_error().decode()}")
        elif has_plan and ix is not None:
            last = open(log).read().rstrip("\n").rsplit("\n", 1)[-1]
            if last.startswith("CASE"):
                return                                         # (nq == 0 and the like: no launch)
            words = dict(kv.split("=", 1) for kv in last.replace(" | ", " ").split(" ", len(NONPTR) + len(PTR) + 3))
            p = ix.last_search_plan()
            want = {k: int(words[k]) for k in p if k in words}
            want.update(blocks=int(words["blocks"]), wpb=int(words["threads"]) // 64, lds=int(words["lds"]), ordered=int(words["perm"]))
            stat["plan_checked"] += 1
            got = {k: p[k] for k in want}
            if got != want or ix.last_search_kernel() != words["kernel"] or p["slots"] != p["blocks"] * p["wpb"]:
                stat["plan_mismatch"].append({"case": name, "plan": got, "line": want, "kernel": ix.last_search_kernel()})

    def checked(f):
        def call():
            try:
                f()
                return 0
            except RuntimeError as e:                          # pg_embedding_amd.check: "<what> failed (<rc>): <text>"
                return int(str(e).split("failed (", 1)[1].split(")", 1)[0])
        return call

    cache = {}

    def index(dim, m, func, n=N_BIG):
        key = (dim, m, func, n)
        if key not in cache:
            if len(cache) >= 6:
                cache.pop(next(iter(cache))).close()
            cache[key] = sp.sparse_index(pg, oracle, dim, m, func, n, seed=dim + m)
        return cache[key]

    def queries(dim, nq):
        return gmm(nq, dim, k=4, seed=dim + 7)

    mine = lambda i: i % nshards == shard                       # noqa: E731
    # 1. the grid at default knobs: dims x ef x m x distance function, one query
    for i, (dim, m, func) in enumerate(itertools.product(DIMS, MS, (0, 1, 2))):
        if mine(i):
            knobs({})
            try:
                ix, Q = index(dim, m, func), queries(dim, 1)
            except ValueError as e:                            # (2000 dims with m = 48: make_meta refuses it, as embedding.c does)
                say(f"CASE grid dim={dim} m={m} func={func}: no such index ({e})")
                continue
            for ef in EFS:
                case(f"grid dim={dim} m={m} func={func} ef={ef}", lambda: sp.batch_dev(ix, Q, ef), ix)
    # 2. launch sizes: both sides of the emulated device's CU count (2), a few blocks, and 300 at narrow widths
    for i, (dim, func) in enumerate(itertools.product(DIMS, (0, 1))):
        if mine(i):
            knobs({})
            ix = index(dim, 12, func)
            for nq, ef in itertools.product((1, 2, 3, 5) + ((300,) if dim in (4, 72, 128) else ()), (16, 100, 200, 400)):
                case(f"nq dim={dim} func={func} nq={nq} ef={ef}", lambda: sp.batch_dev(ix, queries(dim, nq), ef), ix)
    # 3. the knob settings, alone and in the pairs the census uses: dims x ef, L2 (and Manhattan / cosine at three widths)
    for i, (ks, dim) in enumerate(itertools.product(KNOB_SETS, DIMS)):
        if mine(i):
            for func in (0, 1, 2) if dim in (72, 256, 768) else (0,):
                ix, Q = index(dim, 12, func), queries(dim, 5)
                knobs(ks)
                for ef in KNOB_EFS:
                    case(f"knobs {json.dumps(ks, sort_keys=True)} dim={dim} func={func} ef={ef}", lambda: sp.batch_dev(ix, Q, ef), ix)
    # 4. every entry kind, at a narrow and a wide width
    for i, (dim, ef) in enumerate(itertools.product((72, 768), (64, 200))):
        if mine(i):
            entry_kinds(pg, oracle, sp, L, np, case, checked, knobs, say, index, queries, dim, ef)
    # 5. the refused requests
    if mine(0):
        refused(pg, sp, L, np, case, checked, knobs, index, queries)
    knobs({})
    for ix in cache.values():
        ix.close()
    print("AB_WORKER " + json.dumps(stat), flush=True)


def entry_kinds(pg, oracle, sp, L, np, case, checked, knobs, say, index, queries, dim, ef):
    import ctypes as C
    ix, Q = index(dim, 12, 0, 600), queries(dim, 20)
    tag = f"dim={dim} ef={ef}"
    knobs({})
    case(f"kind batch_dev {tag}", lambda: sp.batch_dev(ix, Q[:5], ef), ix)
    case(f"kind caller_order {tag}", lambda: sp.batch_dev(ix, Q[:5], ef, caller_order=True), ix)
    case(f"kind base {tag}", lambda: sp.batch_dev(ix, Q[:5], ef, base=True), ix)
    knobs({"LOCALITY_MIN_NQ": 4})
    case(f"kind ordered {tag}", lambda: sp.batch_dev(ix, Q, ef), ix)
    case(f"kind ordered caller_order {tag}", lambda: sp.batch_dev(ix, Q, ef, caller_order=True), ix)
    o = sp.Out(20, ef)
    ev, tm = np.zeros((20, 64), np.uint32), np.zeros((20, 2), np.uint64)
    case(f"kind traced ordered {tag}", lambda: L.hnsw_gpu_search_traced_dev(ix._h, Q.ctypes.data, 20, ef, *o.args(), ev.ctypes.data, 64, tm.ctypes.data, None), ix)
    knobs({})
    case(f"kind traced {tag}", lambda: L.hnsw_gpu_search_traced_dev(ix._h, Q.ctypes.data, 5, ef, *o.args(), ev.ctypes.data, 64, tm.ctypes.data, None), ix)
    case(f"kind host polled {tag}", checked(lambda: ix.search(Q[:5], ef)), ix)
    case(f"kind host copied {tag}", checked(lambda: ix.search(Q, ef)), ix)
    case(f"kind trace_begin {tag}", checked(lambda: ix.search_trace(Q[0], ef)), ix)
    case(f"kind trace_begin base {tag}", checked(lambda: ix.search_trace(Q[0], ef, base=True)), ix)
    case(f"kind scan {tag}", checked(lambda: ix.scan(Q[:5], 30, ef=16)), ix)
    for fmt, code in (("f16", 1), ("bf16", 2)):
        ix.set_reduced_rows(fmt)
        case(f"kind reduced {fmt} {tag}", lambda: sp.batch_dev(ix, Q[:5], ef, rows=code), ix)
        case(f"kind reduced host {fmt} {tag}", checked(lambda: ix.search(Q[:5], ef, rows=fmt)), ix)
    ix.set_reduced_rows(None)
    ctx = pg.SearchContext(ix)
    for ks, walkers in (({}, 0), ({"TEAM": 1}, 0), ({"TEAM": 1}, 2), ({"TEAM": 1}, 8)):
        knobs(ks)
        ctx.set_walkers(walkers)
        case(f"kind ctx {json.dumps(ks)} walkers={walkers} {tag}", lambda: L.hnsw_gpu_search_batch_ctx(ctx._h, Q.ctypes.data, 5, ef, *o.args(), None))
    ctx.set_walkers(0)
    knobs({})
    case(f"kind ctx flags {tag}", checked(lambda: ctx.search_streamed(Q[:5], ef)))
    case(f"kind ctx host {tag}", checked(lambda: ctx.search_host(Q[:5], ef)))

    def stream(ef_, walkers):
        s = pg.SearchStream(ctx, ef_, ring=64, walkers=walkers)
        s.wait(s.submit(Q[:3]))
        s.close()
    for walkers in (0, 2):
        case(f"kind stream walkers={walkers} {tag}", checked(lambda: stream(ef, walkers)))
    ctx.close()
    # the build's two walks: the batched link step and single inserts
    meta = pg.make_meta(dim, 12, 40, 16, 0)
    b = pg.GpuIndex.empty(meta, 64)
    X = queries(dim, 48)
    b.append(X[:40])
    case(f"kind link {tag}", checked(lambda: b.link(0, 40)), b)
    for j in range(40, 43):
        case(f"kind insert_one {j} {tag}", checked(lambda: b.insert_one(X[j], j)), b)
    b.close()
    sh = pg.LocalShardedIndex.build(X, meta, 2)
    say("CASE kind sharded build done " + tag)
    case(f"kind sharded {tag}", checked(lambda: sh.search(Q[:5], 16)))
    sh.close()
    for s in sh.shards:
        s.close()


def refused(pg, sp, L, np, case, checked, knobs, index, queries):
    ix = index(130, 12, 0, 600)
    Q = queries(130, 5)
    for fmt, code in (("f16", 1), ("bf16", 2)):
        ix.set_reduced_rows(fmt)
        knobs({"BEAM16": 1})
        case(f"refused reduced {fmt} ef=400 dim=130 BEAM16=1", lambda: sp.batch_dev(ix, Q, 400, rows=code), ix)
        case(f"refused reduced host {fmt} ef=400 dim=130 BEAM16=1", checked(lambda: ix.search(Q, 400, rows=fmt)), ix)
        for ks in ({"BEAM": 0}, {"FORCE_LDS_HEAPS": 1}, {"WIDE_EF_MIN": 0}, {"REF_ORDER": 1}):
            knobs(ks)
            case(f"refused reduced {fmt} {json.dumps(ks)}", lambda: sp.batch_dev(ix, Q, 100, rows=code), ix)
        knobs({})
        case(f"refused reduced {fmt} ef=300 dim=130", lambda: sp.batch_dev(ix, Q, 300, rows=code), ix)
    ix.set_reduced_rows(None)
    knobs({"REF_ORDER": 1})
    ix = index(128, 12, 0, 600)
    case("refused REF_ORDER=1 ef=200 dim=128", lambda: sp.batch_dev(ix, queries(128, 5), 200), ix)
    case("accepted REF_ORDER=1 ef=100 dim=128", lambda: sp.batch_dev(ix, queries(128, 5), 100), ix)
    ix = index(72, 12, 0, 600)
    case("refused REF_ORDER=1 L2 dim=72", lambda: sp.batch_dev(ix, queries(72, 5), 100), ix)
    knobs({})
    ctx = pg.SearchContext(ix)
    for ef in (1000, 400):                                     # (1000: refused by hnsw_gpu_stream_open itself; 400 on narrow rows: by the planner)
        case(f"refused stream ef={ef} dim=72", checked(lambda: pg.SearchStream(ctx, ef, ring=64)))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------- driver
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-rev", default="HEAD^")
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", nargs=3, metavar=("LOG", "SHARD", "NSHARDS"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]), int(args.worker[2]))
    import build_emu
    out = build_emu.OUT
    ptree = os.path.join(out, "search_plan_ab_parent")
    subprocess.run(f"rm -rf {ptree} && mkdir -p {ptree} && git archive {args.parent_rev} pg_embedding_amd/csrc | tar -x -C {ptree}", shell=True, check=True, cwd=ROOT)
    libs = {"parent": build_emu.build_tree(os.path.join(ptree, "pg_embedding_amd", "csrc"), "plan_ab_parent", PARENT_EDIT, force=True),
            "this": build_emu.build_tree(tag="plan_ab_this", edit=THIS_EDIT, force=True)}
    procs = []
    for name, lib in libs.items():
        for k in range(args.shards):
            log = os.path.join(out, f"search_plan_ab_{name}_{k}.log")
            if os.path.exists(log):
                os.remove(log)
            procs.append((name, k, log, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", log, str(k), str(args.shards)],
                                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, PGEMB_GPU_LIB=lib, SIMT_EMU_CUS="2"))))
    stats = {}
    for name, k, log, pr in procs:
        o, e = pr.communicate()
        line = [ln for ln in o.splitlines() if ln.startswith("AB_WORKER ")]
        if pr.returncode != 0 or not line:
            for other in procs:
                other[3].kill()
            sys.exit(f"{name} shard {k}: exit {pr.returncode}\n{o[-2000:]}\n{e[-3000:]}")
        stats[(name, k)] = json.loads(line[0][10:])
    lines = {name: [ln for k in range(args.shards) for ln in open(os.path.join(out, f"search_plan_ab_{name}_{k}.log")).read().splitlines()] for name in libs}
    a, b = lines["parent"], lines["this"]
    diff = [(i, x, y) for i, (x, y) in enumerate(itertools.zip_longest(a, b)) if x != y]
    launches = sum(1 for x in a if not x.startswith(("CASE", "RC")))
    kernels = sorted({x.rsplit("kernel=", 1)[1] for x in a if "kernel=" in x})
    mism = [m for (name, k), s in stats.items() for m in s["plan_mismatch"]]
    checked = sum(s["plan_checked"] for (name, k), s in stats.items() if name == "this")
    rep = [f"parent {args.parent_rev} against this tree, SIMT emulator, {args.shards} shards per library",
           f"lines compared: {max(len(a), len(b))} (parent {len(a)}, this tree {len(b)}): {sum(1 for x in a if x.startswith('CASE'))} calls, {launches} search launches, "
           f"{sum(1 for x in a if x.startswith('RC'))} refusals with code and text",
           f"distinct kernels launched: {len(kernels)}",
           f"differing lines: {len(diff)}",
           f"this tree: last_search_plan() / last_search_kernel() checked against the launch's own line after {checked} launches, {len(mism)} mismatches",
           "RESULT: " + ("identical" if not diff and not mism and len(a) == len(b) else "DIFFERENT")]
    for i, x, y in diff[:10]:
        rep += [f"line {i}:", f"  parent: {x}", f"  this:   {y}"]
    for m in mism[:5]:
        rep.append("plan mismatch: " + json.dumps(m))
    print("\n".join(rep))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(rep) + "\n")
    sys.exit(0 if rep[5].endswith("identical") else 1)


if __name__ == "__main__":
    main()
