// The compact target of the leaf handles' sparse Schur entries (pips_hip_ldl_factor_schur_sparse / _batch): the caller owns a symmetric
// Schur complement as one triangle in CSR (the reference's SparseSymmetricMatrix behind hasSparseKkt is the upper one, multMatSymUpper;
// pips_hip_kkt_get_schur_sparse returns the lower one) and the leaves' terms -Br_i^T K_i^-1 Br_i only ever touch the cliques of the
// blocks' non-empty border columns.  The device therefore holds the T distinct pattern positions any clique touches and nothing else:
// the blocks' nb x nb position tables (Engine::set_sc_tables) index into those T doubles, `pos` says where each of them belongs in the
// caller's value array.  Blocks that share Schur columns (x0: all of them, a 2-link row: two) share positions.
// Plain C++ like layout.h and detplan.h: no device call, no environment read; tested without a GPU (pips_schur_target_probe,
// tests/test_schur_target_cpu.py).
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"

namespace pips {

struct SchurTarget {
   std::vector<int> nb;          // per block: non-empty border columns (the rule of schur_pack_block / Engine::border_pack)
   std::vector<long long> off;   // nblk + 1: block b's nb x nb table starts at tab[off[b]]
   std::vector<int> tab;         // entry la * nb + lb, la >= lb: index into pos of the clique pair's place; 0 in the other half
   std::vector<long long> pos;   // the T positions of the caller's value array, ascending
};

// What a later call is compared with instead of a copy of the pattern: its dimension, its entries, the triangle and a 64-bit hash
// (FNV-1a) of the consulted rows - their ids, extents and column indices
struct SchurPatternId {
   int S = 0, lower = 0;
   long long nnz = 0;
   uint64_t hash = 0;
   bool operator==(const SchurPatternId& o) const { return S == o.S && lower == o.lower && nnz == o.nnz && hash == o.hash; }
};

// bt_rowptr[b]: the S + 1 row pointers of block b's border (nullptr: none).  The consulted rows are those of the blocks' non-empty
// border columns (the diagonal counts, so every one of them is read in either triangle).
//   PIPS_ERR_ARG    S <= 0, a consulted row that does not ascend strictly, an extent or a column index out of range
//   PIPS_ERR_STATE  the pattern lacks the entry of a clique pair; the message names it as (row, column) of the pattern
// id only (out == nullptr): the checks of the consulted rows and the hash, no tables
int build_schur_target(int nblk, int S, const int* const* bt_rowptr, const int* sc_rowptr, const int* sc_colidx, int lower, SchurTarget* out,
                       SchurPatternId& id);

}  // namespace pips
