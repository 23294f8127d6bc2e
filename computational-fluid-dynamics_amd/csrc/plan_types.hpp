// plan_types.hpp — what the launch planner (plan.hpp, host only) and the kernels' tile decode share: a strip's
// geometry, the plan structs a launch carries, the small functions both sides evaluate. Host-clean: a plain C++
// compiler takes it (its one HIP include is for __host__ __device__), so tests/plan_check.cpp needs no GPU.
#pragma once

#include <hip/hip_runtime_api.h>

namespace cfd {

// (min / max under names both compilers take; written as HIP's own, so the device code does not move)
__host__ __device__ constexpr int imin(int a, int b) { return (a < b) ? a : b; }
__host__ __device__ constexpr int imax(int a, int b) { return (a > b) ? a : b; }

constexpr int CAVITY = 0, CHANNEL = 1, BACKSTEP = 2;
constexpr int HALO = 8;           // halo rows stored per side (a fused pair of SOR iterations needs 7)

struct Geo {
  int nx, ny;      // global interior cells
  int pitch;       // doubles per stored row
  int row_lo;      // global row index of stored row 0
  int nrows;       // stored rows
  int j0, j1;      // owned interior rows (global, inclusive)
  int wj0, wj1;    // owned rows incl. physical ghost rows on boundary strips
};

constexpr int PAIR_TWC = 128 - 2 * 8;         // output columns per wave (8-column halos)

// Tiling of one pair launch. Rows are covered in up to two ranges [lo0, hi0)
// and [lo1, hi1) (the second may be empty): one launch for a whole strip, or,
// on ranks that overlap the halo exchange, one launch for the interior rows
// and one for the rows next to both neighbours. Every column tile splits each
// range into bands; the first and last column tile (boundary columns, masked
// march) use shorter bands of `the` rows.
struct PairPlan {
  int ctiles;
  int th, nb0, nb1;    // interior column tiles: band height, bands in range 0 / 1
  int the, nbe0, nbe1; // boundary column tiles
  int lo0, hi0, lo1, hi1;
  int cxa, cxb;        // step: column tiles across the step's column (+1; 0: none), banded like the boundary ones
  // step, proof launches (open.hip) only: the block's column tiles. Tiles
  // 1..nl lie left of the step's column, tiles nl+1..nl+ncx cross it (then
  // cxa = cxb = 0: not boundary-class). Below the block, for both: nlf bands
  // of th rows over [lo0, lz) march the interior-column path (away from the
  // block edge), nle bands of `the` rows over [lz, le) the masked one, le =
  // inlet_jmax + 2 (the block's lower edge row included). Above: the left
  // tiles' nlt bands of `the` rows over [lt, hi0) when the range holds ghost
  // row ny + 1 (refreshed from the block's top row; the block's interior rows
  // between never change, both buffers hold them), the crossing tiles' nxt
  // bands over [le, hi0) (fluid right of the block). ncx = 0: no such class.
  int nl, ncx, nlf, nle, nlt, nxt, lz, le, lt;
  // step, reference-order steady launches (lexw.hpp): the crossing column
  // tiles xa .. xa + xn - 1 march their bands xb .. xb + xbn - 1 (those that
  // reach the block's edge: the per-cell solid rules, ~1.7x the cycles per
  // row) as xparts shorter bands, the extra parts' waves after the interior ones
  int xa, xn, xb, xbn, xparts;
};

// column tiles banded as boundary tiles (masked march): the first and last,
// and the step's mixed ones
__host__ __device__ inline int plan_edge_tiles(const PairPlan& pl) {
  return (pl.ctiles >= 2 ? 2 : 1) + (pl.cxa > 0) + (pl.cxb > 0);
}

// waves of a plan (every class)
__host__ __device__ inline int plan_waves(const PairPlan& pl) {
  const int ne = plan_edge_tiles(pl);
  return ne * (pl.nbe0 + pl.nbe1) + pl.nl * (pl.nlf + pl.nle + pl.nlt) + pl.ncx * (pl.nlf + pl.nle + pl.nxt) +
         (pl.ctiles - ne - pl.nl - pl.ncx) * (pl.nb0 + pl.nb1);
}

// Output columns per wave. A value is exact after s half-sweeps on the wave's
// columns [s, 127-s]; the residual evaluated in half-sweep h reads its east
// neighbour's NEW value (column x+1 after h). At 4 sweeps (h up to 8) the last
// output column must therefore be 127-9 = 118: output columns 8..117 (110,
// lanes 4..58; 10-column right halo). Up to 3 sweeps: 8..119 (112, lanes
// 4..59), the red-black kernels' PAIR_TWC. Rows likewise: a strip's stored
// 8-row halo serves up to 3 sweeps (Solver::lexw_ns keeps strips at 3).
// At 5 sweeps (the cavity on one strip) the left halo grows to 10 columns
// (output column 10 reads column 9 after 9 half-sweeps) and the right one to
// 12: output columns 10..115 (106, lanes 5..57). At 6 sweeps (h up to 12) the
// halos are 12 and 14 columns: output columns 12..113 (102, lanes 6..56).
__host__ __device__ constexpr int lexw_twc(int ns) {
  return ns >= 6 ? 102 : ns == 5 ? 106 : ns == 4 ? 110 : PAIR_TWC;
}
__host__ __device__ constexpr int lexw_ch(int ns) { return ns >= 6 ? 12 : ns == 5 ? 10 : 8; }

// Ramp-launch tiling: bands of `th` rows from row `row0`; band b holds the
// column tiles ca..cb (the ones its rows touch), numbered from first: band[b]
// = first << 16 | ca << 8 | cb. Waves map to tiles band by band, column tiles
// side by side (their shared halo columns are read together from one L2),
// with no empty tiles (a workgroup holds its slot until its last wave ends).
constexpr int LEXW_RAMP_BANDS = 256;
struct LexRamp {
  int nb, th, row0;
  int wsplit;  // 1: the wall column tiles (first, last) march each band as two half bands (two waves)
  // the step: its crossing column tiles xa .. xa + xn - 1 march the bands that
  // reach the block's edge (band rows blo .. blo + th - 1 with blo + th + xreach
  // >= jb) as two half bands too (xn = 0: none)
  int xa, xn, xreach;
  unsigned band[LEXW_RAMP_BANDS];
};

// ramp launch: the column tile and half band (-1: the whole band) of wave o of
// a band whose tiles are ca .. cb (split tiles take two consecutive waves)
__host__ __device__ inline int lexw_ramp_waves(const LexRamp& rp, int ctiles, int b, int ca, int cb, int o,
                                               int* ctile, int* half) {
  int sp[4], n = 0;
  if (rp.wsplit && ca == 0 && cb >= ca) sp[n++] = 0;
  if (rp.xn > 0 && rp.row0 + (b + 1) * rp.th + rp.xreach >= 0)
    for (int c = imax(rp.xa, ca); c <= imin(rp.xa + rp.xn - 1, cb); ++c)
      if (c != 0 && c != ctiles - 1) sp[n++] = c;
  if (rp.wsplit && cb == ctiles - 1 && cb > 0) sp[n++] = cb;
  int extra = 0;
  for (int q = 0; q < n; ++q) {
    const int at = sp[q] - ca + extra;
    if (o < at) break;
    if (o == at || o == at + 1) {
      *ctile = sp[q];
      *half = o - at;
      return n;
    }
    ++extra;
  }
  *ctile = ca + o - extra;
  *half = -1;
  return n;  // (the split tiles: the band has cb - ca + 1 + n waves)
}

// A/B build only: every interior band of the open cases on the row-checked
// march (one interior code path in the kernel: is the checked path slow for
// its work or for the instruction cache it shares with the safe path?)
#ifndef CFD_LEXW_ALLRC
#define CFD_LEXW_ALLRC 0
#endif

// Owned rows of column tile `ct` whose output cells launch H0 touches: a cell
// (j,i) is updated in one of the launch's half-sweeps or has its black
// residual of half-sweep H0-1 evaluated (i+j <= H0+2NS-1 and i+j+2(K-1) >=
// H0-1), or finished in the previous launch and must be copied into this
// launch's output buffer (i+j+2(K-1) >= H0-2NS). Other rows hold their final
// values in both buffers already.
// Open cases: the ghost rows / columns too, the left / bottom ghosts active two
// half-sweeps later than their position (lxo_row).
__host__ __device__ inline void lexw_rows(const Geo& g, int H0, int K, int ns, int ct, int* lo, int* hi,
                                          bool open = false) {
  const int twc = lexw_twc(ns);
  if (!open) {
    const int cmin = imax(ct * twc, 1), cmax = imin(ct * twc + twc - 1, g.nx);
    *lo = imax(g.j0, H0 - 2 * ns - 2 * (K - 1) - cmax);
    *hi = imin(g.j1, H0 + 2 * ns - 1 - cmin);
  } else {
    const int cmin = imax(ct * twc, 0), cmax = imin(ct * twc + twc - 1, g.nx + 1);
    *lo = imax(g.wj0, H0 - 2 * ns - 2 * (K - 1) - cmax - 2);
    *hi = imin(g.wj1, H0 + 2 * ns - 1 - cmin);
  }
}

}  // namespace cfd
