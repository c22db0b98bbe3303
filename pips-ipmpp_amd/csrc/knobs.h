// The environment switches of libpipship.so: THE table, one row per switch, and the only readers of the environment (knobs.cpp holds the
// library's one call that reads it).  Plain C++, no HIP include.  DESIGN.md section 10 is generated from this table (tools/knobs_table.py) and
// tests/test_knobs_cpu.py holds every PIPS_HIP_* / PIPS_IPM_* name in the tests, tools and documents against it.
//
// A row: X(identifier, name, kind, default, when it is read, effect).
//   kind   how the value is parsed - the table parses, the caller interprets (clamping stays at the call site):
//            SET   present, with any value (knob_set)
//            INT   atoll of the value, the default where the variable is not set (knob_int)
//            TRI   -1 where it is not set, else whether atoi of the value is non-zero (knob_tri)
//            REAL  atof of the value, the default where it is not set (knob_real)
//            TEXT  the value as it stands, nullptr where it is not set (knob_text)
//   when   create (of the handle), analyze (every analysis), call (every call that takes the path), process (once, at the first use);
//          two of them where the switch has two readers
// Every accessor reads the live environment when it is called and keeps nothing, so a switch is read when the code that asks for it
// runs: a test sets it, analyses, removes it and analyses again.  The exception is the `process` rows: knob_process().
#pragma once

namespace pips {

// clang-format off
#define PIPS_KNOBS(X) \
   X(DETERMINISTIC,      "PIPS_HIP_DETERMINISTIC",      INT,  0,       "create+call",    "non-zero: deterministic mode (section 4.4) for every batch (at creation: the default of pips_hip_batch_set_deterministic) and for the leaf handles' sparse Schur calls") \
   X(MF,                 "PIPS_HIP_MF",                 INT,  1,       "analyze",        "0: scattering head instead of the multifrontal one") \
   X(MF_SPLIT,           "PIPS_HIP_MF_SPLIT",           INT,  176,     "analyze",        "border split: 0 off, else only up to that many border columns (2 ... 176)") \
   X(MF_KONLY,           "PIPS_HIP_MF_KONLY",           INT,  0,       "analyze",        "non-zero: fronts on the rows of K only, border rows formed afterwards in gather form (section 4.1c; slower)") \
   X(MF_LDS,             "PIPS_HIP_MF_LDS",             INT,  19200,   "analyze",        "LDS budget of a front in doubles (tests: small values force the update matrices into device memory)") \
   X(MF_CLOCKS,          "PIPS_HIP_MF_CLOCKS",          SET,  0,       "call",           "set to any value: per-front phase clocks on stderr, at every factorisation") \
   X(SN_WIDTH,           "PIPS_HIP_SN_WIDTH",           INT,  16,      "analyze",        "symbolic analysis: supernode width cap (1 ... 32; not set: the handle's setting, else 16)") \
   X(RELAX_ZEROS,        "PIPS_HIP_RELAX_ZEROS",        REAL, 0.4,     "analyze",        "symbolic analysis: admissible share of explicit zeros in an amalgamated panel") \
   X(ND_DEPTH,           "PIPS_HIP_ND_DEPTH",           INT,  12,      "analyze",        "symbolic analysis: dissection levels (0 = off)") \
   X(ND_MIN,             "PIPS_HIP_ND_MIN",             INT,  128,     "analyze",        "symbolic analysis: smallest segment that is still dissected (with the three above: how the tests reach the chain / spine / wide-supernode paths)") \
   X(SCHUR_MODE,         "PIPS_HIP_SCHUR_MODE",         INT,  0,       "analyze",        "1 / 2: the Schur mode of an analysis whose caller left it to the cost model - the leaf handles and the batch they are bound into have no setter (tests of pips_hip_ldl_factor_schur_sparse / _batch)") \
   X(SPINE,              "PIPS_HIP_SPINE",              TRI,  -1,      "analyze",        "solve sweeps: spine kernels off / on (not set: where the head has a spine)") \
   X(MULTI,              "PIPS_HIP_MULTI",              INT,  1,       "call",           "solve sweeps of several right-hand sides: 0 one by one, any other value interleaved on the matrix pipe from two on (2: whole panels, 4: half panels, whatever the size); not set: interleaved from 8 on") \
   X(SWEEP_LAUNCHES,     "PIPS_HIP_SWEEP_LAUNCHES",     SET,  0,       "create+analyze", "set to any value: tail sweeps launch by launch instead of the single-launch kernels (leaf batch: at analysis, dense root: at creation)") \
   X(SWEEP_POLL_LIMIT,   "PIPS_HIP_SWEEP_POLL_LIMIT",   INT,  4000000, "create+analyze", "polls before a waiting workgroup of a single-launch sweep gives up") \
   X(BORDER_BACKWARD,    "PIPS_HIP_BORDER_BACKWARD",    TRI,  -1,      "analyze",        "Ltsolve from the augmented factor off / on instead of the cost rule") \
   X(AUG_SWEEPS,         "PIPS_HIP_AUG_SWEEPS",         TRI,  -1,      "analyze",        "solveCompressed by sweeps of the augmented factor off / on whatever the cost model says") \
   X(AUG_WITNESS,        "PIPS_HIP_AUG_WITNESS",        INT,  1,       "create",         "0: the refined pass as the witness of the augmented sweeps on one rank too (section 2)") \
   X(TAIL_SINGLE,        "PIPS_HIP_TAIL_SINGLE",        TRI,  -1,      "analyze",        "the leaf tails as one dependency-driven launch off / on whatever the batch size (section 4.2a; not set: up to 16 blocks)") \
   X(TAIL_TRACE,         "PIPS_HIP_TAIL_TRACE",         TEXT, 0,       "call",           "a file: per-task clocks of the single tail launch (tools/tail_trace.py), at every factorisation") \
   X(TAIL_FIRST_TOUCH,   "PIPS_HIP_TAIL_FIRST_TOUCH",   TRI,  -1,      "analyze",        "0: the tails cleared and added to (k_arena_clear, k_root_assemble) instead of written once, assembled (section 4.1; not set: first touch where the batch allows it)") \
   X(FIRST_TOUCH_LDS,    "PIPS_HIP_FIRST_TOUCH_LDS",    INT,  81920,   "analyze",        "bytes of LDS a first-touch tail column may take (0 ... 163840; the tests refuse the path with a small value)") \
   X(TAIL_PANEL,         "PIPS_HIP_TAIL_PANEL",         INT,  1,       "call",           "0: leaf tails of more than 16 blocks tile column by tile column (tail_columns) instead of group by group (tail_panels, section 4.2): A/B runs, and the test that compares the two entry for entry") \
   X(TRSM_DENSE,         "PIPS_HIP_TRSM_DENSE",         INT,  0,       "call",           "non-zero: trsm of the leaf tails in the static pivot order with the dense product instead of the triangular one (k_tile_gemm modes 1 / 5, section 4.2), and the column launches with it: A/B runs, and the test that compares the two entry for entry") \
   X(DUMP_SN,            "PIPS_HIP_DUMP_SN",            TEXT, 0,       "call",           "a file: one line per head supernode (width, rows, level, parent), written by pips_symbolic_probe") \
   X(ROOT_LAUNCHES,      "PIPS_HIP_ROOT_LAUNCHES",      SET,  0,       "create",         "set to any value: dense root, static order: launch per step instead of the single launch (section 4.3)") \
   X(ROOT_CHAIN_CU,      "PIPS_HIP_ROOT_CHAIN_CU",      TRI,  -1,      "call",           "dense root, single launch: 0 one task list, the chain wherever its workgroups land (A/B); read when the launch's plan is built, at the root's first factorisation") \
   X(ROOT_DIAG_BARRIERS, "PIPS_HIP_ROOT_DIAG_BARRIERS", INT,  0,       "analyze+call",   "non-zero: the 128-barrier diagonal tile instead of the blocked one, in the single tail launch (at analysis) and the dense root's single launch (at every factorisation)") \
   X(ROOT_POLL_LIMIT,    "PIPS_HIP_ROOT_POLL_LIMIT",    INT,  400000,  "analyze+call",   "polls before a wait inside the dense root's single launch gives up (read with its plan, at the first factorisation); the single tail launch takes 50 times as many (at analysis)") \
   X(ROOT_TRACE,         "PIPS_HIP_ROOT_TRACE",         TEXT, 0,       "call",           "a file: per-task clocks of every single-launch root factorisation (tools/root_trace.py, tools/root_diag_phases.py)") \
   X(ROOT_DISTRIBUTED,   "PIPS_HIP_ROOT_DISTRIBUTED",   INT,  0,       "create",         "non-zero, several ranks: the dense root factorised column-cyclically over the ranks instead of redundantly on each") \
   X(DIST_NO_LOOKAHEAD,  "PIPS_HIP_DIST_NO_LOOKAHEAD",  SET,  0,       "call",           "set to any value: the distributed dense root without its second stream (test)") \
   X(ROOT_SYNC,          "PIPS_HIP_ROOT_SYNC",          SET,  0,       "process",        "set to any value: the root, dense or sparse, factorised on the main stream instead of its own") \
   X(SPARSE_ROOT_ASYNC,  "PIPS_HIP_SPARSE_ROOT_ASYNC",  INT,  1,       "process",        "0: the sparse root factorised on the main stream instead of its own (section 4.3b); per handle: pips_hip_kkt_set_root_stream") \
   X(SPARSE_ROOT_BAND,   "PIPS_HIP_SPARSE_ROOT_BAND",   INT,  0,       "create",         "order of the sparse root: 0 minimum degree, 1 dense-tile band, 2 dissected around the hubs (section 4.3b); not set: chosen by the tile envelope") \
   X(SC_PANELS,          "PIPS_HIP_SC_PANELS",          INT,  0,       "create",         "several ranks: row panels of the Schur reduction (1 = one reduction after all leaf work); not set: 4 from S = 4096 on, else 1") \
   X(SC_REDUCE,          "PIPS_HIP_SC_REDUCE",          TEXT, 0,       "create",         "rsag: reduce-scatter + all-gather instead of the all-reduce of the Schur complement") \
   X(FORCE_REDUCE,       "PIPS_HIP_FORCE_REDUCE",       SET,  0,       "create",         "set to any value: the reduction path with a single rank (tests)") \
   X(IPM_SPARSE_ROOT,    "PIPS_IPM_SPARSE_ROOT",        INT,  0,       "create",         "device IPM harness: non-zero: sparse root") \
   X(IPM_ROOT_INEQ_ELIMINATE, "PIPS_IPM_ROOT_INEQ_ELIMINATE", TRI, -1, "create",         "device IPM harness: root inequality rows kept / eliminated (not set: eliminated with the dense root only)") \
   X(IPM_SCHUR_MODE,     "PIPS_IPM_SCHUR_MODE",         TEXT, 0,       "create",         "device IPM harness: the leaves' Schur mode, 0 auto, 1 augmented factorisation, 2 blocked solves, deterministic mode included (section 4.4); not set: the batch's default, mode 1 with the sparse root")
// clang-format on

enum Knob : int {
#define X(id, name, kind, dflt, when, effect) K_##id,
   PIPS_KNOBS(X)
#undef X
   K_COUNT
};
enum KnobKind : int { KNOB_SET, KNOB_INT, KNOB_TRI, KNOB_REAL, KNOB_TEXT };
struct KnobRow { const char* name; KnobKind kind; double dflt; const char* when; const char* effect; };
inline constexpr KnobRow KNOBS[K_COUNT] = {
#define X(id, name, kind, dflt, when, effect) {name, KNOB_##kind, dflt, when, effect},
   PIPS_KNOBS(X)
#undef X
};

// the readers behind the accessors (knobs.cpp); the accessors check the kind where they are compiled
const char* knob_raw(Knob k);     // the variable's value, nullptr where it is not set: the library's one read of the environment
long long knob_raw_int(Knob k);   // atoll of it, else the row's default
int knob_raw_tri(Knob k);         // -1, else atoi of it != 0
double knob_raw_real(Knob k);     // atof of it, else the row's default

// whether the variable is there at all: the whole value of a SET switch, and what tells "not set" from a value for a switch of
// another kind whose caller keeps its own rule for that case
template <Knob K> inline bool knob_set() { return knob_raw(K) != nullptr; }
template <Knob K> inline long long knob_int() { static_assert(KNOBS[K].kind == KNOB_INT, "not an INT switch"); return knob_raw_int(K); }
template <Knob K> inline int knob_tri() { static_assert(KNOBS[K].kind == KNOB_TRI, "not a TRI switch"); return knob_raw_tri(K); }
template <Knob K> inline double knob_real() { static_assert(KNOBS[K].kind == KNOB_REAL, "not a REAL switch"); return knob_raw_real(K); }
template <Knob K> inline const char* knob_text() { static_assert(KNOBS[K].kind == KNOB_TEXT, "not a TEXT switch"); return knob_raw(K); }

// The `process` rows: read once, when the first root factorisation of the process asks, and never again - a test that sets one of them
// later in its process runs the default.
struct ProcessKnobs { bool root_sync; bool sparse_root_async; };
const ProcessKnobs& knob_process();

}  // namespace pips
