// Plain records and constants shared by the host layout pass (layout.cpp) and the kernels (kernels.hip.h): what the host fills
// and the device reads.  No HIP include: this header compiles with a plain C++ compiler.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PIPS_HD __host__ __device__
#else
#define PIPS_HD
#endif

namespace pips {

constexpr int TILE = 128;

struct SnDesc {
   long long panel;  // global arena offset of the ld x w panel
   long long rows;   // global offset into rowidx
   long long upd;    // global offset into upd (head-to-head update segments)
   int w, r, c0, blk;
   int n_useg, rb;   // number of update segments; index of the first border row among the r below-rows
   int ld, pad_;     // leading dimension of the stored panel: w + r, or w + rb for a front under the border split (its border rows live
                     // only in the border-row arena at bb: Lt[k * rpb + a - rb], rpb = r - rb rounded up to 4)
   long long slot;   // deterministic mode: first contribution slot of the factorisation scatter (r (r + 1) / 2 slots: pair (a, b),
                     // a >= b, has slot + b r - b (b - 1) / 2 + a - b)
   long long vslot;  // ... and of the forward-substitution scatter (r slots)
   long long U;      // multifrontal head: offset of the packed r x r update matrix inside the update arena, -1 if none
   long long mf;     // multifrontal head: offset of the front record inside mfint (common.h "Front record"), -1 for simple leaves
   long long bb;     // border split: offset of the supernode's border rows inside the border-row arena (k_border_schur), -1 if none
};

struct BlkDesc {
   long long arena_off;  // block arena base (doubles)
   long long T;          // global arena offset of the tail panel
   long long sncol_off;  // offset into sn_of_col (values are global supernode ids)
   long long xw_off;     // offset of the permuted work vector (length n_head + m_pad)
   long long x_off;      // offset into flat original-order vectors (sum of n over preceding blocks)
   long long bmap_off;   // offset into bmap
   long long winv_off;   // offset into winv (ntc tiles of TILE*TILE)
   long long dt_off;     // offset into dtail (m_pad)
   long long sctab_off;  // offset of this block's nb x nb position table inside sctab (sparse Schur complement), else 0
   int n, n_head, m, m_pad, nb, nb_pad, ldT, ntc, ntr;
   int mf_split;         // multifrontal head with the border split (BlockSym::mf_split)
   long long U;          // offset of the block's scaled tail copy U = L D (m_pad x m_pad, ld = m_pad) inside the U arena
   double thr_rel, repl_rel;  // pivot threshold / replacement relative to the pivot's reference magnitude pref[k]
   double repl_abs;           // replacement when no reference magnitude exists (structurally zero diagonal)
   long long lv_off;          // multifrontal head: offset of the block's leaf values inside the leaf-value arena
   long long k_off, b_off;    // offsets of the block's K values / border values (Engine::d_kval, d_bval): k_front reads its panel entries there
   long long T_in;            // where the tail panel is ASSEMBLED (scatter, root fronts, border rows of the head) and accumulated: = T when the tail is
                              // factorised in place (launch per step), a scratch region behind the panels when it is one launch (tailkernel.hip.h)
};

struct TileTask { int blk, ti, tj, pad; };
struct TileStrip { int off, cnt; };   // k_tile_panel: the tasks [off, off + cnt) of one tile row, in the order they run
struct TaskList { long long off = 0; int cnt = 0; };   // a launch's tasks: a range of a task array
// kind of a task of the single-launch factorisations (rootkernel.hip.h, tailkernel.hip.h)
constexpr int ROOT_UPD = 0, ROOT_TRSM = 1, ROOT_DIAG = 2;

constexpr int HEAD_WMAX = 32;   // widest head supernode (solve kernels)
constexpr int SIMPLE_RMAX = 16;

constexpr int BB_GMAX = 8;
// register tile of k_border_schur: BB_TR rows x 4 columns of L_b D L_b^T per thread and step (BB_TR = 4: square tiles over the lower triangle;
// 8: two row groups per tile - six LDS reads per 32 multiply-adds instead of four per 16)
constexpr int BB_TR = 4;
// tiles of a supernode with rp (a multiple of 4) padded border rows; tile t -> (column group tb of 4, row group ta of BB_TR)
PIPS_HD inline int bb_tile_count(int rp) {
   const int nt4 = rp >> 2;
   if (BB_TR == 4) return nt4 * (nt4 + 1) / 2;
   const int nt8 = (rp + 7) >> 3;
   int cnt = 0;
   for (int tb = 0; tb < nt4; ++tb) cnt += nt8 - (tb >> 1);
   return cnt;
}
struct BbMeta { int lt_off, pos_off, w, nbj, tile0, pad0, pad1, pad2; };   // staging offset of Lt (doubles; the pivots follow at + w * rp),
                                                                          // offset of the rows' positions inside the batch's list, tiles before it
struct BbBatch {
   long long src;     // offset of the batch inside the border-row arena
   long long pos;     // offset of its rows' positions (compressed border ids) inside bbpos
   int first, cnt;    // its supernodes inside the BbMeta array
   int ndoubles, ntiles, npos, pad;
};

// Backward substitution of the simple leaves from a compact record (24 bytes instead of the 88-byte SnDesc + BlkDesc the general
// kernel reads - on the time-coupled blocks the descriptors were most of this kernel's traffic): x_c = x_c / d - sum_a l_a x[rows_a]
struct LeafDesc {
   long long panel;   // d, l_0 .. l_{r-1} in the arena
   int rows;          // offset into rowidx
   int xoff;          // the block's offset in the work vector
   int c0;            // the leaf's column (block-local, permuted)
   int r_in;          // rows inside the block (the border rows behind them take no part in solves with K_i)
};

// Entry of the deterministic forward sweep of the augmented factor (k_border_rowdot_det): where the w factors of the row lie (stride
// between them) and the first of the supernode's columns in the work vector.
struct BgEntry { long long off; unsigned y; unsigned short stride, w; };

// First touch of the tails (k_tail_first_touch; layout.h "first-touch plan"), per tail column.
// An entry of K or of the border that lands in the column: its row inside the tail panel and its place in the value array
// (src >= 0: K value src; src < 0: border value ~src).
struct FtInit { int row, src; };
// One column b of a root front's update matrix: cnt entries from uarena[u], going to the rows rowidx[rows .. rows + cnt)
struct FtPiece {
   long long u, rows;
   int cnt, front;   // front: the root front's supernode id (pieces of a column ascend by it)
};

constexpr int FULL_LONG_ROW = 512;

static_assert(sizeof(FtInit) == 8 && sizeof(FtPiece) == 24, "record layout read by the kernels");
static_assert(sizeof(SnDesc) == 96 && sizeof(BlkDesc) == 176 && sizeof(TileTask) == 16, "record layout read by the kernels");
static_assert(sizeof(BbMeta) == 32 && sizeof(BbBatch) == 40 && sizeof(LeafDesc) == 24 && sizeof(BgEntry) == 16, "record layout read by the kernels");

}  // namespace pips
