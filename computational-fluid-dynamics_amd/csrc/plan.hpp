// plan.hpp — the SOR launch planner: band heights, tile classes, ramp tables, steady windows and the plan
// report (cfd_sor_plan_info), as free functions over an explicit input (PlanIn). Host only and pure - no HIP,
// no Solver, no global state - so any grid's plans can be checked without a GPU (tests/plan_check.cpp).
// solver.hip keeps the wave budgets (occupancy queries) and enqueues what these functions plan.
#pragma once

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/cfd_amd.h"
#include "plan_types.hpp"

// 1: the reference order's ramp launches march the wall column tiles as two
// half bands each (lexw.hpp LexRamp::wsplit): the wall tiles' masked march set
// the ramp launches' time (per-launch stamps); cavity 4096^2 704-717 -> 717-729
// GLUPS, channel and 1024^2 neutral to +0.5 % (profiles/r4_lexw_stamps)
#ifndef CFD_LEXW_WALL_SPLIT
#define CFD_LEXW_WALL_SPLIT 1
#endif
// the step's crossing column tiles: the bands at the block's edge as this many shorter bands (1: no split)
#ifndef CFD_LEXW_XSPLIT
#define CFD_LEXW_XSPLIT 3
#endif

namespace cfd {

constexpr int MARCH_MIN_TH = 24;   // minimum rows per band of a wave-march launch
constexpr int OVL_ROWS = 16;       // rows next to each neighbour updated by the overlapped boundary launch

// What the planner reads: the grid and case (cfd_params), the strips, the knobs (cfd_set_tuning), the split defaults
struct PlanIn {
  int case_id = CFD_CAVITY, nx = 0, ny = 0;
  int step_i = 0, inlet_jmax = 0;  // backwards step: the block is i <= step_i, j > inlet_jmax
  int n_strips = 1;
  int pair_edge_pct = 45;          // boundary-column band length, % of the interior march (open cases; cavity: 80)
  int lexw_edge_pct = 100;         // reference order: wall-tile band length, % of the interior band (default: 75 up to 2048 rows)
  int march_min_th = MARCH_MIN_TH;
  int march_order = 0;             // CFD_TUNE_MARCH_ORDER (the report only)
  int lexw_ramp_pct = 0;           // ramp launches: bands at least this % of the steady plan's (CFD_TUNE_LEXW_RAMP_PCT)
  bool lexw_left = true;           // backwards step: the left column tiles' class (CFD_TUNE_LEXW_LEFT)
  bool lexw_updown = true;         // cavity steady launches: odd interior bands march up (CFD_TUNE_LEXW_UPDOWN)
  int wall_split = CFD_LEXW_WALL_SPLIT, xsplit = CFD_LEXW_XSPLIT;
};

// What multi_plan / wave_bands know about a plan beyond the PairPlan itself (cfd_sor_plan_info)
struct PlanNote {
  int waves = 0, sweeps = 0, extra = 0, max_th = 1 << 30, tiles = 0;
  bool budget_bands = false, shortened = false;
  int clamped = 0;
};

// Sizing of the wave-march kernels: column tiles of `twc` output columns,
// each split into bands so that one resident round covers the strip.
inline void wave_bands(const PlanIn& in, int rows, int twc, int resident, int& ctiles, int& th, int& nbands) {
  ctiles = (in.nx + 2 + twc - 1) / twc;
  const int per_tile = std::max(1, resident / (ctiles * in.n_strips));
  const int bands = std::max(1, std::min(per_tile, (rows + in.march_min_th - 1) / in.march_min_th));
  th = (rows + bands - 1) / bands;
  nbands = (rows + th - 1) / th;
}
// the report's view of wave_bands: one class of ctiles x nbands tiles over the strip's rows
inline PairPlan wave_report(const PlanIn& in, const Geo& g, int resident, int ctiles, int th, int nbands, PlanNote& nt) {
  const int rows = g.wj1 - g.wj0 + 1;
  PairPlan pw{};
  pw.ctiles = ctiles;
  pw.th = pw.the = th;
  pw.nb0 = pw.nbe0 = nbands;
  pw.lo0 = g.wj0; pw.hi0 = g.wj1 + 1;
  nt.waves = resident / in.n_strips;
  nt.sweeps = 1;
  nt.extra = 0;
  nt.tiles = ctiles * nbands;
  nt.budget_bands = std::max(1, resident / (ctiles * in.n_strips)) < (rows + in.march_min_th - 1) / in.march_min_th;
  return pw;
}

// an n-sweep launch that runs open.hip's proof march (its plans may carry the step's left class)
inline bool open_proof_n(const PlanIn& in, int n, bool proof_launch) {
  return in.case_id != CFD_CAVITY && n >= 3 && proof_launch;
}
// Rows one interior wave marches beyond its band (both sides together, plus
// the parity alignment row) for an n-sweep launch: the cavity's pipeline has
// depth 2n+1, the open cases' pair pipeline 7.
inline int march_extra(const PlanIn& in, int n) { return (in.case_id == CFD_CAVITY || n == 4) ? 2 * (2 * n + 1) + 1 : 15; }
// Tiling of an n-sweep launch over rows [lo0, hi0) + [lo1, hi1) with at most
// `waves` waves (one resident round). Interior column tiles: bands of th
// rows, marched in groups of 10 over th + march_extra rows, so th + extra is
// a multiple of 10. The two boundary column tiles march slower (masks):
// shorter bands, pair_edge_pct % of the interior march.
// left_class (the step's proof launches, open.hip): the column tiles over
// the step's block (left of its column and across it) become their own
// class (PairPlan::nl / ncx): interior-path bands below the block, short
// masked bands next to its lower edge and above it.
// note (optional): what cfd_sor_plan_info reports about the plan (written, never read here)
inline PairPlan multi_plan(const PlanIn& in, int lo0, int hi0, int lo1, int hi1, int waves, int n, int max_th = 1 << 30,
                           int edge_pct = -1, int twc = PAIR_TWC, int ex = -1, bool left_class = false,
                           PlanNote* note = nullptr) {
  if (edge_pct < 0) edge_pct = in.pair_edge_pct;
  PairPlan pl{};
  pl.ctiles = (in.nx + 2 + twc - 1) / twc;
  pl.lo0 = lo0; pl.hi0 = hi0; pl.lo1 = lo1; pl.hi1 = hi1;
  if (in.case_id == CFD_BACKSTEP) {
    // interior column tiles across the step's column (neither left of it,
    // kernels.hpp: c0 + 128 <= step_i - 1, nor right, c0 > step_i + 1) march
    // with per-cell masks: band them like the boundary tiles
    int nx_found = 0;
    for (int ct = 1; ct + 1 < pl.ctiles && nx_found < 2; ++ct) {
      const int c0 = ct * PAIR_TWC - 8;
      if (!(c0 > in.step_i + 1) && !(c0 + 128 <= in.step_i - 1)) {
        (nx_found == 0 ? pl.cxa : pl.cxb) = ct + 1;
        ++nx_found;
      }
    }
  }
  const int rows = (hi0 - lo0) + (hi1 - lo1);
  const int rmax = std::max(hi0 - lo0, hi1 - lo1);
  if (ex < 0) ex = march_extra(in, n);
  auto nbands = [](int lo, int hi, int t) { return hi > lo ? (hi - lo + t - 1) / t : 0; };
  // the block's column class (PairPlan::nl / ncx): column tiles 1 .. cxa-2
  // (wholly left of the step's column) and the crossing ones; rows [lo0, lz)
  // interior-column bands (every row the march reads below the block's
  // lower edge row: open.hip cols_in), [lz, le) short masked bands, above
  // that the top ghost row (left tiles) or every row (crossing tiles)
  const int cx_last = pl.cxb > 0 ? pl.cxb - 1 : pl.cxa - 1;  // the last crossing tile
  const bool lc = left_class && in.case_id == CFD_BACKSTEP && pl.cxa > 1 && cx_last < pl.ctiles - 1 && hi1 <= lo1;
  if (lc) {
    pl.nl = pl.cxa - 2;
    pl.ncx = pl.cxb > 0 ? 2 : 1;
    pl.cxa = pl.cxb = 0;  // (the crossing tiles leave the boundary class)
    pl.lz = std::max(lo0, std::min(hi0, in.inlet_jmax - (2 * n + 2)));
    pl.le = std::max(pl.lz, std::min(hi0, in.inlet_jmax + 2));
    pl.lt = hi0;  // (ghost row ny + 1 in the range: set with `the` below)
  }
  auto left_bands = [&] {
    if (!lc) return;
    pl.nlf = nbands(lo0, pl.lz, pl.th);
    pl.nle = nbands(pl.lz, pl.le, pl.the);
    if (hi0 == in.ny + 2) pl.lt = std::max(pl.le, hi0 - pl.the);
    pl.nlt = nbands(pl.lt, hi0, pl.the);
    pl.nxt = nbands(pl.le, hi0, pl.the);
  };
  int nb = std::max(1, std::min(waves / std::max(1, pl.ctiles), (rows + in.march_min_th - 1) / in.march_min_th));
  nb = std::max(nb, (rows + max_th - 1) / max_th);
  const int nb_first = nb;
  bool clamped = false;
  for (;; --nb) {  // most interior bands whose tiles (boundary tiles included) fit one round
    pl.th = std::max(1, std::min(rmax, ((rows + nb - 1) / nb + ex + 9) / 10 * 10 - ex));
    if (pl.th > max_th) {  // (lexw: one wave marches at most max_th rows)
      pl.th = max_th;
      pl.the = std::max(8, std::min(rmax, (pl.th + ex) * edge_pct / 100 - ex));
      pl.nb0 = nbands(lo0, hi0, pl.th);
      pl.nb1 = nbands(lo1, hi1, pl.th);
      pl.nbe0 = nbands(lo0, hi0, pl.the);
      pl.nbe1 = nbands(lo1, hi1, pl.the);
      left_bands();
      clamped = true;
      break;
    }
    pl.the = std::max(8, std::min(rmax, (pl.th + ex) * edge_pct / 100 - ex));
    pl.nb0 = nbands(lo0, hi0, pl.th);
    pl.nb1 = nbands(lo1, hi1, pl.th);
    pl.nbe0 = nbands(lo0, hi0, pl.the);
    pl.nbe1 = nbands(lo1, hi1, pl.the);
    left_bands();
    if (plan_waves(pl) <= waves || nb == 1) break;
  }
  if (note) {
    note->waves = waves;
    note->sweeps = n;
    note->extra = ex;
    note->max_th = max_th;
    note->tiles = plan_waves(pl);
    note->budget_bands = waves / std::max(1, pl.ctiles) < (rows + in.march_min_th - 1) / in.march_min_th;
    note->shortened = nb < nb_first;
    note->clamped = clamped ? 1 : (pl.th == rmax && ((pl.th + ex) % 10) != 0) ? 2 : 0;
  }
  return pl;
}

// a rank's boundary launch beside its halo exchange: one band next to each neighbour (lo_b / hi_b rows: 0 at a wall)
inline PairPlan overlap_boundary_plan(const PlanIn& in, const Geo& g, int lo_b, int hi_b) {
  PairPlan pb{};
  pb.ctiles = (in.nx + 2 + PAIR_TWC - 1) / PAIR_TWC;
  pb.th = pb.the = OVL_ROWS;
  pb.lo0 = g.wj0; pb.hi0 = g.wj0 + lo_b;
  pb.lo1 = g.wj1 + 1 - hi_b; pb.hi1 = g.wj1 + 1;
  pb.nb0 = pb.nbe0 = lo_b ? 1 : 0;
  pb.nb1 = pb.nbe1 = hi_b ? 1 : 0;
  return pb;
}

// ---- lexicographic order, multi-block (lexw.hpp) ----
// rows one lexw wave marches beyond its band: the pipeline (2NS+1 each side) + parity row
inline int lexw_extra(int ns) { return 2 * (2 * ns + 1) + 1; }
inline int lexw_offset(const PlanIn& in) { return (in.nx + in.ny) / 2 + 192; }
inline int floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
// iterations whose residual every cell has contributed after launch m (H0 = 2 + 2NS m)
inline int lexw_done(const PlanIn& in, int m, int ns) {
  return m < 0 ? 0 : floordiv(2 + 2 * ns * m + 2 * ns - 2 - in.nx - in.ny, 2) + 1;
}
// launches of a K-iteration solve: the last covers the last half-sweep - cell (ny, nx)'s K-th update, and for
// the open cases the top ghost (ny+1, nx)'s K-th copy one half-sweep later (lxo_row)
inline int lexw_launches(const PlanIn& in, int ns, int K) {
  const int Hlast = in.nx + in.ny + 2 * (K - 1) + (in.case_id != CFD_CAVITY ? 1 : 0);
  return (Hlast - 2) / (2 * ns) + 1;
}
// a strip's steady plan (a wave's march steps + 9 <= 127, its iterations fit one 64-bit mask; 6 sweeps: 90 + 27 + 9)
inline PairPlan lexw_steady_plan(const PlanIn& in, const Geo& g, int waves, int ns, PlanNote* note) {
  return multi_plan(in, g.wj0, g.wj1 + 1, 0, 0, waves, ns, ns >= 5 ? 90 : 96, in.lexw_edge_pct, lexw_twc(ns),
                    lexw_extra(ns), false, note);
}

// steady launches of a strip: every cell the strip's launch touches (its
// rows and the HALO rows on each side: i + j in [smin, smax]) active in
// every half-sweep of the launch and of the previous one's last
// (smax + 1 <= H0 <= smin + 2K - 2NS - 1, H0 = 2 + 2NS m; one strip:
// smin = 2, smax = nx + ny). A strip of a tall grid (ranks) runs its own
// steady window instead of the whole grid's, which starts only once the
// last row has started. Launches *m0 .. *m1 (empty: *m1 < *m0).
inline void lexw_steady_window(const PlanIn& in, const Geo& g, int ns, int K, int* m0, int* m1) {
  const int smax = in.nx + std::min(in.ny, g.j1 + HALO), smin = 1 + std::max(1, g.j0 - HALO);
  *m0 = (smax - 1 + 2 * ns - 1) / (2 * ns);
  *m1 = floordiv(smin + 2 * K - 2 * ns - 3, 2 * ns);
}

// steady: every cell active in every half-sweep of the launch and in the
// previous launch's last one (no activity masks: the leaner kernel)
// backwards step, reference order: the block's ghost constants set before
// the march (lexw.hpp step_presolid_kernel), so that the column tiles left
// of the step's column end at the block's bottom row and march as a channel
// below it (flags bit 3; CFD_TUNE_LEXW_LEFT 0: the per-cell masked march)
inline bool lexw_left_class(const PlanIn& in) { return in.case_id == CFD_BACKSTEP && in.lexw_left; }
// the step's interior column tiles that cross its column (the per-cell solid
// rules at the block's edge): xa .. xa + xn - 1, xa = -1 if none
inline void lexw_cross_tiles(const PlanIn& in, int ns, const PairPlan& pl, int* xa, int* xn) {
  const int twc = lexw_twc(ns), ch = lexw_ch(ns), si = in.step_i;
  *xa = -1;
  *xn = 0;
  for (int ct = 1; ct + 1 < pl.ctiles; ++ct) {
    const int c0 = ct * twc - ch;
    const bool left = c0 + 127 <= si - 1 && lexw_left_class(in);
    if (!left && c0 <= si + 1) {
      if (*xa < 0) *xa = ct;
      *xn = ct - *xa + 1;
    }
  }
}

// cfd_sor_plan_info, host only: which marches poisson_lexw_kernel's decode gives the tiles of a
// launch - the kernel's own tests restated (lexw.hpp), so that the report says what ran.
// An interior band [y0, y1) of a plain open-case column tile is row-checked (never marched up):
inline bool lexw_row_checked(const PlanIn& in, int ns, const Geo& g, int y0, int y1, bool left) {
  const int H = 2 * ns + 1;
  const int rmin = std::max(g.row_lo, 0);
  int rmax = std::min(g.row_lo + g.nrows - 1, g.ny + 1);
  const int jg = left ? in.inlet_jmax + 1 : g.ny + 1;
  if (left) rmax = std::min(rmax, in.inlet_jmax + 2);
  return CFD_LEXW_ALLRC || !(y0 - H + 1 > rmin && y1 + H + 2 * ns < std::min(rmax, jg));
}
// a steady launch: the interior column tiles of the step's left class, and the odd interior bands
// that march up in the plain interior column tiles (neither left class nor crossing)
inline void lexw_steady_classes(const PlanIn& in, int ns, const PairPlan& pl, const Geo& g, bool updown, int* left_tiles,
                                int* up_bands) {
  const int twc = lexw_twc(ns), ch = lexw_ch(ns);
  int nleft = 0, plain = 0;
  for (int ct = 1; ct + 1 < pl.ctiles; ++ct) {
    const int c0 = ct * twc - ch;
    if (in.case_id != CFD_BACKSTEP) ++plain;
    else if (c0 + 127 <= in.step_i - 1 && lexw_left_class(in)) ++nleft;
    else if (c0 > in.step_i + 1) ++plain;
  }
  int up = 0;
  if (updown && plain > 0)
    for (int b = 1; b < pl.nb0 + pl.nb1; b += 2) {
      const bool r0 = b < pl.nb0;
      const int y0 = r0 ? pl.lo0 + b * pl.th : pl.lo1 + (b - pl.nb0) * pl.th;
      const int y1 = std::min(y0 + pl.th, r0 ? pl.hi0 : pl.hi1);
      if (y0 < y1 && (in.case_id == CFD_CAVITY || !lexw_row_checked(in, ns, g, y0, y1, false))) ++up;
    }
  *left_tiles = nleft;
  *up_bands = up;
}
// a ramp launch: does some tile take the upward march (an odd band's whole-band interior tile,
// wholly active in every half-sweep the launch evaluates, unmasked and unchecked)?
inline bool lexw_ramp_up(const PlanIn& in, int ns, const PairPlan& pl, const Geo& g, const LexRamp& rp,
                         const std::vector<std::pair<int, int>>& rr, int H0, int K) {
  const bool open = in.case_id != CFD_CAVITY;
  const int H = 2 * ns + 1, twc = lexw_twc(ns), ch = lexw_ch(ns), glo = open ? 0 : 1;
  const int Hend = H0 + 2 * ns - 1, last = 2 * (K - 1) + (open ? 2 : 0);
  for (int b = 1; b < rp.nb; b += 2) {
    const unsigned e = rp.band[b];
    const int ca = (e >> 8) & 255, cb = e & 255;
    const bool xsplit = rp.xn > 0 && rp.row0 + (b + 1) * rp.th + rp.xreach >= 0;  // (lexw_ramp_waves: half bands)
    for (int c = std::max(ca, 1); c <= std::min(cb, pl.ctiles - 2); ++c) {
      if (xsplit && c >= rp.xa && c < rp.xa + rp.xn) continue;
      const int y0 = std::max(rp.row0 + b * rp.th, rr[c].first);
      int y1 = std::min(rp.row0 + (b + 1) * rp.th, rr[c].second + 1);
      const int c0 = c * twc - ch;
      bool left = false;
      if (in.case_id == CFD_BACKSTEP && c0 + 127 <= in.step_i - 1 && lexw_left_class(in)) {
        left = c0 >= 1;
        y1 = std::min(y1, in.inlet_jmax + 2);
      }
      if (y0 >= y1) continue;
      const int rlo = std::max(std::max(y0 - H - 1, glo), g.row_lo);
      const int rhi = std::min(std::min(y1 + H, g.ny + 1 - glo), g.row_lo + g.nrows - 1);
      const int clo = std::max(c0, glo), chi = std::min(c0 + 127, g.nx + 1 - glo);
      const int smin = clo + rlo, smax = chi + rhi;
      if (smin > Hend || smax + last < H0 - 2 * ns) continue;
      if (!(open ? (c0 >= 1 && c0 + 127 <= g.nx) : (clo == c0 && chi == c0 + 127))) continue;  // (cols_in)
      if (!open) {
        if (smax <= H0 - 2 && Hend <= smin + last) return true;
        continue;
      }
      if (in.case_id == CFD_BACKSTEP && !left) {
        const int jb = in.inlet_jmax + 1, si = in.step_i;
        if (c0 + 127 <= si - 1 && y0 - H - 1 >= jb + 1 && y1 + H + 2 * ns + 1 <= g.ny) continue;  // (solids only)
        if (y1 + H + 2 * ns + 1 >= jb - 1 && c0 <= si + 1) continue;                               // (the general tiles)
      }
      if (!lexw_row_checked(in, ns, g, y0, y1, left) && smax <= H0 - 2 && Hend <= smin + 2 * (K - 1)) return true;
    }
  }
  return false;
}

// What one reference-order launch of plan pl runs (half-sweeps from H0 of a K-iteration solve, at most `waves`
// tiles): the tile count (0: no launch), the ramp table, the plan with the step's steady split, the rules that fired
struct LexLaunch {
  int ntiles = 0;
  LexRamp rp{};
  PairPlan plx{};
  std::vector<std::pair<int, int>> rr;  // ramp launches: the rows each column tile touches (lexw_rows)
  bool by_floor = false, grown_bands = false, grown_tiles = false, fell_back = false;
  bool too_wide = false;  // more column tiles or tiles than the ramp table's fields hold: not launchable
};
inline LexLaunch lexw_launch_plan(const PlanIn& in, int ns, bool steady, const PairPlan& pl, const Geo& g, int H0, int K,
                                  int waves) {
  LexLaunch out;
  out.plx = pl;
  const int ne = pl.ctiles >= 2 ? 2 : 1;
  int ntiles = ne * (pl.nbe0 + pl.nbe1) + (pl.ctiles - ne) * (pl.nb0 + pl.nb1);
  LexRamp& rp = out.rp;
  if (!steady) {
    // ramp launch: tile only the rows it touches (lexw_rows), bands of the
    // shortest height whose tiles fit one resident round, at most the
    // steady plan's (at that every ramp launch fits: it touches fewer rows)
    int rl = 1 << 30, rh = -1;
    long long tot = 0;
    std::vector<std::pair<int, int>>& rr = out.rr;
    rr.resize(pl.ctiles);
    for (int c = 0; c < pl.ctiles; ++c) {
      lexw_rows(g, H0, K, ns, c, &rr[c].first, &rr[c].second, in.case_id != CFD_CAVITY);
      if (rr[c].second >= rr[c].first) {
        rl = std::min(rl, rr[c].first);
        rh = std::max(rh, rr[c].second);
        tot += rr[c].second - rr[c].first + 1;
      }
    }
    if (rh < rl) return out;
    const int ex = lexw_extra(ns);
    rp.wsplit = in.wall_split;
    if (in.case_id == CFD_BACKSTEP && in.xsplit > 1) {  // the step's crossing tiles (as the steady split)
      int xa, xn;
      lexw_cross_tiles(in, ns, pl, &xa, &xn);
      if (xa >= 0) {
        rp.xa = xa;
        rp.xn = xn;
        rp.xreach = 4 * ns + 4 - (in.inlet_jmax + 1);
      }
    }
    auto build = [&](int th) {  // fills rp for band height th; returns the tile count
      rp.th = th;
      rp.row0 = rl;
      rp.nb = (rh - rl) / th + 1;
      int n = 0;
      for (int b = 0; b < rp.nb; ++b) {
        const int blo = rl + b * th, bhi = blo + th - 1;
        int ca = -1, cb = -2;
        for (int c = 0; c < pl.ctiles; ++c)
          if (std::max(blo, rr[c].first) <= std::min(bhi, rr[c].second)) {
            if (ca < 0) ca = c;
            cb = c;
          }
        if (ca < 0) ca = 0, cb = -1;  // (an empty band: no tiles)
        rp.band[b] = ((unsigned)n << 16) | ((unsigned)ca << 8) | (unsigned)(cb < 0 ? 0 : cb);
        if (cb < 0) rp.band[b] = ((unsigned)n << 16) | 1u << 8;  // ca 1 > cb 0: empty
        n += std::max(0, cb - ca + 1);
        if (cb >= ca) {  // a second wave per split tile (lexw_ramp_waves: half bands)
          int ct, hf;
          n += lexw_ramp_waves(rp, pl.ctiles, b, ca, cb, 0, &ct, &hf);
        }
      }
      return n;
    };
    int th = (int)std::max<long long>(1, (tot + waves - 1) / std::max(1, waves));
    // (a floor on the band height trades idle wave slots for less pipeline fill per output row)
    out.by_floor = pl.th * in.lexw_ramp_pct / 100 > th;  // (by_floor .. fell_back: cfd_sor_plan_info)
    th = std::max(th, pl.th * in.lexw_ramp_pct / 100);
    th = std::max(1, (th + ex + 9) / 10 * 10 - ex);
    while ((rh - rl) / th + 1 > LEXW_RAMP_BANDS) {
      th += 10;
      out.grown_bands = true;
    }
    ntiles = build(th);
    while (th < pl.th && ntiles > waves) {
      ntiles = build(th += 10);
      out.grown_tiles = true;
    }
    if (th > pl.th) {
      ntiles = build(th = std::max(pl.th, (rh - rl) / LEXW_RAMP_BANDS + 1));
      out.fell_back = true;
    }
    out.too_wide = pl.ctiles > 255 || ntiles >= 65536;
  }
  // the step's steady launches: the crossing column tiles' bands that reach
  // the block's edge as CFD_LEXW_XSPLIT shorter bands (lexw.hpp; they set
  // the launch's time: profiles/r5/step_8192x512_lex_stamps.json)
  PairPlan& plx = out.plx;
  if (steady && in.case_id == CFD_BACKSTEP && in.xsplit > 1 && pl.nb1 == 0 && pl.ctiles >= 3) {
    const int jb = in.inlet_jmax + 1;
    int xa, xn;
    lexw_cross_tiles(in, ns, pl, &xa, &xn);
    int xb = -1;
    for (int b = 0; b < pl.nb0 && xb < 0; ++b)
      if (std::min(pl.lo0 + (b + 1) * pl.th, pl.hi0) + 4 * ns + 4 >= jb) xb = b;
    if (xa >= 0 && xb >= 0) {
      plx.xa = xa;
      plx.xn = xn;
      plx.xb = xb;
      plx.xbn = pl.nb0 - xb;
      plx.xparts = in.xsplit;
      ntiles += plx.xn * plx.xbn * (plx.xparts - 1);
    }
  }
  out.ntiles = ntiles;
  return out;
}

// cfd_sor_plan_info: the plans of the most recent solve, noted where its launches are planned (nothing reads it back)
struct PlanReport {
  cfd_sor_plan rep{};
  // the entry of a plan in rep.plan (appended at its first launch; nullptr: the table is full)
  cfd_sor_band_plan* entry(const PlanIn& in, int kind, const PairPlan& pl, const PlanNote& nt, bool proof) {
    cfd_sor_band_plan b{};
    b.kind = kind;
    b.sweeps = nt.sweeps;
    b.proof = proof ? 1 : 0;
    b.waves = nt.waves;
    b.lo0 = pl.lo0; b.hi0 = pl.hi0; b.lo1 = pl.lo1; b.hi1 = pl.hi1;
    b.ctiles = pl.ctiles;
    b.th = pl.th; b.nb0 = pl.nb0; b.nb1 = pl.nb1;
    b.the = pl.the; b.nbe0 = pl.nbe0; b.nbe1 = pl.nbe1;
    b.nl = pl.nl; b.ncx = pl.ncx;
    b.tiles = nt.tiles;
    b.extra = nt.extra;
    b.max_th = nt.max_th;
    b.budget_bands = nt.budget_bands;
    b.shortened = nt.shortened;
    b.clamped = nt.clamped;
    b.march_order = kind == CFD_PLAN_LEXW ? 0 : in.march_order;
    for (int q = 0; q < rep.n_plans; ++q) {
      const cfd_sor_band_plan& a = rep.plan[q];
      if (a.kind == b.kind && a.sweeps == b.sweeps && a.proof == b.proof && a.waves == b.waves && a.lo0 == b.lo0 &&
          a.hi0 == b.hi0 && a.lo1 == b.lo1 && a.hi1 == b.hi1 && a.th == b.th && a.the == b.the && a.nb0 == b.nb0 &&
          a.nbe0 == b.nbe0 && a.tiles == b.tiles && a.march_order == b.march_order)
        return &rep.plan[q];
    }
    if (rep.n_plans == CFD_SOR_PLAN_MAX) {
      ++rep.plans_dropped;
      return nullptr;
    }
    rep.plan[rep.n_plans] = b;
    return &rep.plan[rep.n_plans++];
  }
  // a launch enqueued with the plan (the red-black kinds)
  void launched(const PlanIn& in, int kind, const PairPlan& pl, const PlanNote& nt, bool proof) {
    if (cfd_sor_band_plan* b = entry(in, kind, pl, nt, proof)) ++b->launches;
  }
  // a reference-order launch of plan pl as lexw_launch_plan laid it out (sample: sampled residual rows)
  void lexw_launched(const PlanIn& in, int ns, bool steady, bool sample, const PairPlan& pl, const PlanNote& nt,
                     const Geo& g, const LexLaunch& ll, int H0, int K) {
    cfd_sor_band_plan* const rb = entry(in, CFD_PLAN_LEXW, pl, nt, false);
    if (ll.ntiles <= 0) return;
    if (!steady) {
      ++rep.ramp_launches;
      rep.ramp_th_min = rep.ramp_th_min ? std::min(rep.ramp_th_min, ll.rp.th) : ll.rp.th;
      rep.ramp_th_max = std::max(rep.ramp_th_max, ll.rp.th);
      rep.ramp_nb_max = std::max(rep.ramp_nb_max, ll.rp.nb);
      rep.ramp_tiles_max = std::max(rep.ramp_tiles_max, ll.ntiles);
      ++(ll.by_floor ? rep.ramp_by_floor : rep.ramp_by_budget);
      rep.ramp_grown_bands += ll.grown_bands;
      rep.ramp_grown_tiles += ll.grown_tiles;
      rep.ramp_fallback += ll.fell_back;
      if (in.lexw_updown && sample && !rep.ramp_up) rep.ramp_up = lexw_ramp_up(in, ns, pl, g, ll.rp, ll.rr, H0, K) ? 1 : 0;
    } else if (rb) {  // (what this steady launch runs)
      ++rb->launches;
      rb->launch_tiles = ll.ntiles;
      rb->xn = ll.plx.xn;
      rb->xbn = ll.plx.xbn;
      lexw_steady_classes(in, ns, pl, g, in.lexw_updown && sample, &rb->left_tiles, &rb->up_bands);
    }
  }
};

}  // namespace cfd
