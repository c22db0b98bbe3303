// Which columns of a pips_hip_kkt_solve_compressed_multi call go together (KktSystem::solve_compressed_multi in kkt.hip.h).  Plain C++
// like tileplan.h: no device call, no environment read - the threshold and the chunk bound come in as numbers; tested without a GPU
// (pips_kkt_multi_plan_probe, tests/test_solve_multi_reference_cpu.py).
#pragma once
#include <algorithm>
#include <vector>

namespace pips {

struct KktMultiChunk {
   int first, count, path;   // columns [first, first + count); path 0: the single solveCompressed, column by column; 1: panels
};

constexpr long long KKT_MULTI_BUDGET_BYTES = 2LL << 30;   // the Ltsolve's panel W = Br X0: n_total x chunk doubles
constexpr int KKT_MULTI_CHUNK_MIN = 32;                    // one panel of the matrix-pipe sweeps: never fewer columns per chunk

// columns a chunk may hold: whole panels of 32 within the budget for n_total x chunk doubles, at most chunk_max, never below 32
inline int kkt_multi_chunk_cap(int chunk_max, long long n_total, long long budget_bytes) {
   const long long per_col = std::max<long long>(n_total, 1) * (long long)sizeof(double);
   const long long fit = budget_bytes / per_col / KKT_MULTI_CHUNK_MIN * KKT_MULTI_CHUNK_MIN;
   return (int)std::max<long long>(KKT_MULTI_CHUNK_MIN, std::min<long long>(std::max(chunk_max, KKT_MULTI_CHUNK_MIN), fit));
}

// from: the fewest right-hand sides that go by panels (Engine::multi_knob().from; 0 = never).  n_total: the longest leaf vector of any
// rank (every rank must cut the same chunks: each chunk ends in one collective)
inline std::vector<KktMultiChunk> kkt_multi_plan(int nrhs, int from, int chunk_max, long long n_total, long long budget_bytes) {
   std::vector<KktMultiChunk> out;
   if (nrhs <= 0) return out;
   if (from <= 0 || nrhs < from) {
      for (int q = 0; q < nrhs; ++q) out.push_back({q, 1, 0});
      return out;
   }
   const int cap = kkt_multi_chunk_cap(chunk_max, n_total, budget_bytes);
   for (int q = 0; q < nrhs; q += cap) out.push_back({q, std::min(cap, nrhs - q), 1});
   return out;
}

}   // namespace pips
