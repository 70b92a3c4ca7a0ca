"""The census of the search kernels: one entry per instantiation of hnsw_search_kernel_beam / _wide / _lds and rerank_kernel that
libhnsw_gpu.so contains (csrc/search_kernels.h + csrc/search_inst.hip spell them out), with the launch that reaches it.

Written from the rules of plan_search and search_kernel_of (csrc/gpu_search.hip), not from a run:

  load shape     shape_index(kiters), kiters = ceil(ceil4(dims) / 64): <= 128 floats Shape2x4 (Shape2x2 for the hot narrow form),
                 <= 256 Shape4x2, <= 512 Shape8x2, wider Shape12x2
  set registers  ef <= 64: 2, <= 128: 4, <= 256: 8, <= 512: 16 — the last by default only on Shape8x2 / Shape12x2, on narrower
                 rows with HNSW_GPU_BEAM16=1
  team           HNSW_GPU_TEAM=1 / 0 (by default it depends on the row width and the launch size)
  Shape2x2       <= 128 floats, 2 / 4 set registers, L2 / Manhattan, not a team (HNSW_GPU_NARROW5=0: the Shape2x4 kernel instead);
                 its lean form unless HNSW_GPU_LEAN=0
  reference      HNSW_GPU_REF_ORDER=1: function codes 3 (L2) / 5 (cosine) / 4 (Manhattan), 4 set registers, one wave per query;
                 L2 needs dims % 16 == 0, cosine / Manhattan dims % 4 == 0, ef <= 128
  wide           ef > HNSW_GPU_WIDE_EF_MIN (default 2048; 0 = every ef)
  generic        HNSW_GPU_FORCE_LDS_HEAPS=1; its sets in HBM when HNSW_GPU_LDS_SET_MIN_WAVES waves of them do not fit the LDS of a CU
  reduced rows   search(rows="f16" | "bf16"): ShapeR16<format, ...> by the same shape index, one wave per query, 2 / 4 / 8 set
                 registers, 16 only on the two wider shapes; then rerank_kernel<function, the fp32 shape>

Every entry names two row widths of its shape: the first ends a load batch inside the row (72: 18 of the batch's 32 chunks; 130 and
260: an odd kiters, so the last 256-byte reduced block carries one real and one zero chunk, and the only batch of Shape4x2 resp. Shape8x2
is short, as is that of ShapeR16<., 4, 2, 4> at 260 (3 of 4 blocks); 520: kiters 9 = one short batch of Shape12x2, 5 reduced blocks; 1000: a full
batch and a short one), the second fills its batches.  The reference-order kernels need dims % 16 == 0 for L2, which none of the tail widths has, and
Shape12x2 has no such width among 520 / 1000: they run at 128 / 256 / 512 / 768 against the compiled reference.

A new instantiation needs an entry here (tests/test_kernel_census_host.py compares this table with the library's symbols), and
tests/test_gpu_kernel_census.py launches every entry and compares last_search_kernel() with its name, character for character;
tests/test_search_plan_emu.py does the same on the emulated library, with the plan's invariants."""
from collections import namedtuple

L2, COSINE, MANHATTAN = 0, 1, 2
FUNCS = (L2, COSINE, MANHATTAN)
REF_CODE = {L2: 3, COSINE: 5, MANHATTAN: 4}               # device_dist.h: F_L2_REF, F_COSINE_REF, F_MANHATTAN_REF
FMT_CODE = {"f16": 1, "bf16": 2}                           # include/hnsw_gpu.h HNSW_GPU_ROWS_*

SHAPES = ("Shape2x4", "Shape4x2", "Shape8x2", "Shape12x2")                # by shape_index
RSHAPES = ("1, 4, 4", "2, 4, 4", "4, 2, 4", "6, 2, 2")                   # ShapeR16<format, KB, RPG, MIN_WAVES> by shape_index
DIMS = ((72, 128), (130, 256), (260, 512), (520, 1000))                   # (tail case, full-batch case) by shape_index
REF_DIMS = ((128,), (256,), (512,), (768,))                               # reference order: dims % 16 == 0
EF_OF_SETS = {2: 16, 4: 100, 8: 200, 16: 400}
LAUNCH_SIZES = (1, 300)

# every HNSW_GPU_* variable an entry may set; a launch of the census starts from none of them set
KNOBS = ("HNSW_GPU_TEAM", "HNSW_GPU_NARROW5", "HNSW_GPU_LEAN", "HNSW_GPU_BEAM16", "HNSW_GPU_FORCE_LDS_HEAPS",
         "HNSW_GPU_LDS_SET_MIN_WAVES", "HNSW_GPU_WIDE_EF_MIN", "HNSW_GPU_REF_ORDER")

# name: as last_search_kernel() prints it (= the demangled symbol without its argument list); form: beam | team | narrow | reference |
# wide | generic | reduced | rerank; dims: the row widths to run it at; func: the index's distance function; fmt: None | "f16" | "bf16"
Entry = namedtuple("Entry", "name form dims func ef fmt env")


def shape_index(dims):
    """device_dist.h shape_index(kiters) of an index of `dims` floats per row (stride = dims rounded up to 4 floats)"""
    kiters = ((dims + 3) // 4 + 15) // 16
    return 0 if kiters <= 2 else 1 if kiters <= 4 else 2 if kiters <= 8 else 3


def set_registers(ef):
    return 2 if ef <= 64 else 4 if ef <= 128 else 8 if ef <= 256 else 16 if ef <= 512 else None


def _b(v):
    return "true" if v else "false"


def _beam(func_code, shape, sets, team, lean):
    return f"pgemb::hnsw_search_kernel_beam<{func_code}, pgemb::{shape}, {sets}, {_b(team)}, {_b(lean)}>"


def _entries():
    out = []
    for s, shape in enumerate(SHAPES):
        for f in FUNCS:
            for sets, ef in EF_OF_SETS.items():
                b16 = {"HNSW_GPU_BEAM16": "1"} if sets == 16 and s < 2 else {}
                # one wave per query.  On rows of <= 128 floats L2 / Manhattan with 2 / 4 set registers would take Shape2x2.
                env = {"HNSW_GPU_TEAM": "0", **b16}
                if s == 0 and f != COSINE and sets <= 4:
                    env["HNSW_GPU_NARROW5"] = "0"
                out.append(Entry(_beam(f, shape, sets, False, False), "beam", DIMS[s], f, ef, None, env))
                out.append(Entry(_beam(f, shape, sets, True, False), "team", DIMS[s], f, ef, None, {"HNSW_GPU_TEAM": "1", **b16}))
            out.append(Entry(_beam(REF_CODE[f], shape, 4, False, False), "reference", REF_DIMS[s], f, 100, None, {"HNSW_GPU_REF_ORDER": "1"}))
            out.append(Entry(f"pgemb::hnsw_search_kernel_wide<{f}, pgemb::{shape}>", "wide", DIMS[s], f, 100, None, {"HNSW_GPU_WIDE_EF_MIN": "0"}))
            out.append(Entry(f"pgemb::hnsw_search_kernel_lds<{f}, pgemb::{shape}, false>", "generic", DIMS[s], f, 100, None,
                             {"HNSW_GPU_FORCE_LDS_HEAPS": "1"}))
            out.append(Entry(f"pgemb::hnsw_search_kernel_lds<{f}, pgemb::{shape}, true>", "generic", DIMS[s], f, 200, None,
                             {"HNSW_GPU_FORCE_LDS_HEAPS": "1", "HNSW_GPU_LDS_SET_MIN_WAVES": "1000"}))
    for f in (L2, MANHATTAN):                                  # the hot narrow-row form and its lean variant
        for sets in (2, 4):
            out.append(Entry(_beam(f, "Shape2x2", sets, False, True), "narrow", DIMS[0], f, EF_OF_SETS[sets], None, {"HNSW_GPU_TEAM": "0"}))
            out.append(Entry(_beam(f, "Shape2x2", sets, False, False), "narrow", DIMS[0], f, EF_OF_SETS[sets], None,
                             {"HNSW_GPU_TEAM": "0", "HNSW_GPU_LEAN": "0"}))
    for s, rshape in enumerate(RSHAPES):
        for f in FUNCS:
            for fmt, code in FMT_CODE.items():
                for sets, ef in EF_OF_SETS.items():
                    if sets == 16 and s < 2:
                        continue                               # not instantiated: REFUSED below
                    out.append(Entry(_beam(f, f"ShapeR16<{code}, {rshape}>", sets, False, False), "reduced", DIMS[s], f, ef, fmt, {}))
    for s, shape in enumerate(SHAPES):                          # not reported by last_search_kernel(): the reduced searches of (func, shape) run it
        for f in FUNCS:
            out.append(Entry(f"pgemb::rerank_kernel<{f}, pgemb::{shape}>", "rerank", DIMS[s], f, None, None, {}))
    return out


ENTRIES = _entries()

# instantiations no public call plus knob reaches: (name, one line of reason).  None: the team form's LDS carve leaves a memo of
# >= 256 entries and >= 3 waves per block at every width and set size above (m = 12), and the dispatcher refuses no reduced-row kernel
# that exists.
UNREACHABLE = ()

# requests the dispatcher refuses with HNSW_GPU_ERR_ARG before any launch, because the kernel does not exist: 16 set registers on the
# reduced-row walks of the two narrower shapes.  (dims, ef, env)
REFUSED_REDUCED = ((130, 400, {"HNSW_GPU_BEAM16": "1"}),)


def names():
    return [e.name for e in ENTRIES]


def entries_for(dims, func, forms=None):
    return [e for e in ENTRIES if dims in e.dims and e.func == func and (forms is None or e.form in forms)]
