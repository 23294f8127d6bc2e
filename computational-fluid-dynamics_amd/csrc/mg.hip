// mg.hip — kernels of the multigrid pressure solve (mg.hpp).
//
// Levels too large for one workgroup run as plain fp64 streams over a level's
// own rows (128-B aligned, cell (j, i) at j * pitch + i): each wave takes one
// row x 128 columns, a lane the 16-B aligned column pair (gi, gi + 1). The
// sweeps of one smoothing step are one launch from p to a second buffer, each
// workgroup running them on an LDS tile with recomputed halos
// (mg_smooth_tile_kernel); the plain form is one launch per colour, in place
// (mg_smooth_kernel: a colour's cells read only the other colour's, so no
// launch reads what it writes), kept for comparison. The residual is
// formed inside the restriction (the children of a coarse cell) and the
// coarse correction's ghost layer inside the prolongation, so neither goes to
// memory. From the first level whose cells fit one workgroup's LDS down, the
// whole sub-cycle - smoothing, restriction, the coarsest level's SOR sweeps,
// prolongation - is one launch of one workgroup (mg_tail_kernel): those levels
// are launch-bound, and the arithmetic is the same per-cell functions.
//
// Every kernel is one template over a scheme: a struct of static per-cell
// functions over its level type (mg.hpp) - the update of a cell, the coarse
// source of a coarse cell, the correction of a fine cell, whether a cell is an
// unknown. The file states the five schemes' cell functions first (the
// cavity's mg_*, the channel's mgo_*, the step's mgs_*, the any-size cavity's
// mga_*, the any-size channel's mgoa_*, each in the operand order of its
// restatement under tests/), then the kernels, then the launches.
// What only the step needs - the fluid tests and the coupled pair A / B - sits
// behind `if constexpr (S::has_pair)` or folds away with S::unknown.
// The library builds with -ffp-contract=off: no fused multiply-adds.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mg.hpp"

namespace cfd {

namespace {

constexpr int MG_TR = 64, MG_TC = 128, MG_TILE_THREADS = 1024, MG_TQ = MG_TR / 16;  // the smoothing tile (below)

// ============================================================= the cavity ==
// Operand order (tests/mg_reference.py, cavity-01.cpp:651-654, 670-673): the
// indicator products are real multiplies on boundary cells (0 * x keeps x's
// sign, as in the reference); interior cells skip them (1 * x == x), the same
// bits.

__device__ __forceinline__ bool mg_interior(const MgLevel* L, int j, int i) {
  return i > 1 && i < L->nx && j > 1 && j < L->ny;
}

struct MgCoef {
  double ew, ee, en, cs;
  int idx;
};
__device__ __forceinline__ MgCoef mg_coef(const MgLevel* L, int j, int i) {
  MgCoef k;
  const int w = i > 1, e = i < L->nx, n = j < L->ny, r1 = j == 1;
  k.ew = w ? 1.0 : 0.0;
  k.ee = e ? 1.0 : 0.0;
  k.en = n ? 1.0 : 0.0;
  k.cs = r1 ? L->cS : 1.0;
  k.idx = w | e << 1 | n << 2 | r1 << 3;
  return k;
}

// Gauss-Seidel update of cell (j, i): rdiag ((ee pE + ew pW) + (en pN + cs pS) - f h2)
__device__ __forceinline__ double mg_relax(const MgLevel* L, int j, int i, double pW, double pE, double pS, double pN,
                                           double f) {
  if (mg_interior(L, j, i)) return L->rdiag[7] * (((pE + pW) + (pN + pS)) - f * L->h2);
  const MgCoef k = mg_coef(L, j, i);
  return L->rdiag[k.idx] * (((k.ee * pE + k.ew * pW) + (k.en * pN + k.cs * pS)) - f * L->h2);
}

// SOR update of the coarsest level, the reference's form: p (1 - w) + (w rdiag) (...)
__device__ __forceinline__ double mg_sor(const MgLevel* L, int j, int i, double pc, double pW, double pE, double pS,
                                         double pN, double f) {
  const MgCoef k = mg_coef(L, j, i);
  return pc * L->one_m_omega + L->omr[k.idx] * (((k.ee * pE + k.ew * pW) + (k.en * pN + k.cs * pS)) - f * L->h2);
}

// residual ih2 (ee (pE - c) + ew (pW - c) + en (pN - c) + cs (pS - c)) - f
__device__ __forceinline__ double mg_resid(const MgLevel* L, int j, int i, double c, double pW, double pE, double pS,
                                           double pN, double f) {
  if (mg_interior(L, j, i)) return L->ih2 * ((((pE - c) + (pW - c)) + (pN - c)) + (pS - c)) - f;
  const MgCoef k = mg_coef(L, j, i);
  return L->ih2 * (((k.ee * (pE - c) + k.ew * (pW - c)) + k.en * (pN - c)) + k.cs * (pS - c)) - f;
}

// Coarse source of cell (J, I) from a[r][c] = p(2J-2+r, 2I-2+c) (the corners
// unused) and f of the four children (fSW = f(2J-1, 2I-1), ...).
__device__ __forceinline__ double mg_restrict_cell(const MgLevel* Lf, int J, int I, const double (&a)[4][4], double fSW,
                                                   double fSE, double fNW, double fNE) {
  const int j = 2 * J - 1, i = 2 * I - 1;
  const double rSW = mg_resid(Lf, j, i, a[1][1], a[1][0], a[1][2], a[0][1], a[2][1], fSW);
  const double rSE = mg_resid(Lf, j, i + 1, a[1][2], a[1][1], a[1][3], a[0][2], a[2][2], fSE);
  const double rNW = mg_resid(Lf, j + 1, i, a[2][1], a[2][0], a[2][2], a[1][1], a[3][1], fNW);
  const double rNE = mg_resid(Lf, j + 1, i + 1, a[2][2], a[2][1], a[2][3], a[1][2], a[3][2], fNE);
  return -0.25 * ((rSW + rSE) + (rNW + rNE));
}

// e of the coarse level with one ghost layer: north ghost = row ny, south
// ghost = row 1 times g, then west / east ghosts = the adjacent column.
__device__ __forceinline__ double mg_ext(const MgLevel* Lc, const double* e, int pitch, int J, int I) {
  const int ii = min(max(I, 1), Lc->nx);
  if (J == 0) return e[(size_t)pitch + ii] * Lc->g;
  if (J == Lc->ny + 1) return e[(size_t)Lc->ny * pitch + ii];
  return e[(size_t)J * pitch + ii];
}

// bilinear correction of fine cell (j, i): (((9 c + 3 V) + 3 H) + D) / 16, V / H / D the
// coarse neighbours on the child's side (south for odd j, west for odd i)
__device__ __forceinline__ double mg_corr(const MgLevel* Lc, const double* e, int pitch, int j, int i) {
  const int J = (j + 1) >> 1, I = (i + 1) >> 1;
  const int dj = (j & 1) ? -1 : 1, di = (i & 1) ? -1 : 1;
  const double c = e[(size_t)J * pitch + I];
  const double V = mg_ext(Lc, e, pitch, J + dj, I);
  const double H = mg_ext(Lc, e, pitch, J, I + di);
  const double D = mg_ext(Lc, e, pitch, J + dj, I + di);
  return (((9.0 * c + 3.0 * V) + 3.0 * H) + D) * 0.0625;
}

// What a scheme supplies to the kernels (the others below alike). A field is a pointer with rows of P
// doubles, global memory or LDS.
struct MgCavity {
  using Level = MgLevel;
  static constexpr bool has_pair = false;   // no coupled pair of cells A / B
  static constexpr bool pair_loads = true;  // the colour launch reads aligned double2 pairs
  // whether cell (j, i) inside the grid is an unknown
  static __device__ __forceinline__ bool unknown(const Level*, int, int) { return true; }
  static __device__ __forceinline__ double relax(const Level* L, int j, int i, double pW, double pE, double pS, double pN,
                                                 double f) {
    return mg_relax(L, j, i, pW, pE, pS, pN, f);
  }
  // the update of cell (j, i), p pointing at it: Gauss-Seidel, or the coarsest level's SOR
  static __device__ __forceinline__ double update(const Level* L, const double* p, int P, int j, int i, double f, bool sor) {
    return sor ? mg_sor(L, j, i, p[0], p[-1], p[1], p[-P], p[P], f) : mg_relax(L, j, i, p[-1], p[1], p[-P], p[P], f);
  }
  // the source of cell (J, I) of level Lf + 1 from Lf's fields. Global rows are 128-B aligned and column
  // 2I - 2 even: two aligned pairs per row; LDS rows of nx + 2 doubles are not 16-B aligned: scalar loads.
  template <bool Aligned>
  static __device__ __forceinline__ double coarse_source(const Level* Lf, const double* p, const double* f, size_t P, int J,
                                                         int I) {
    const size_t o = (size_t)(2 * J - 2) * P + (size_t)(2 * I - 2);
    double a[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (Aligned) {
        const double2 lo = *reinterpret_cast<const double2*>(p + o + r * P);
        const double2 hi = *reinterpret_cast<const double2*>(p + o + r * P + 2);
        a[r][0] = lo.x, a[r][1] = lo.y, a[r][2] = hi.x, a[r][3] = hi.y;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) a[r][c] = p[o + r * P + c];
      }
    }
    return mg_restrict_cell(Lf, J, I, a, f[o + P + 1], f[o + P + 2], f[o + 2 * P + 1], f[o + 2 * P + 2]);
  }
  // the correction of cell (j, i) of level L from e of level L + 1 (rows of `pitch` doubles)
  static __device__ __forceinline__ double corr(const Level* L, const double* e, int pitch, int j, int i) {
    return mg_corr(L + 1, e, pitch, j, i);
  }
};

// ============================================================ the channel ==
// The second scheme (mg.hpp "the channel", tests/mg_open_reference.py): an
// anisotropic, semi-coarsened operator with a Dirichlet zero in the east ghost
// column. A neighbour a cell does not have is skipped by a
// select on the cell's mask (bit set: the neighbour exists), never multiplied
// by 0, so the ghost cells - which hold the reference's refreshed values at
// level 0 and nothing in particular elsewhere - reach no result.

__device__ __forceinline__ int mgo_mask(const MgoLevel* L, int j, int i) {
  return (int)(i > 1) | (int)(i < L->nx) << 1 | (int)(j > 1) << 2 | (int)(j < L->ny) << 3;
}

// (cx pE + cx pW) + (cy pN + cy pS) over the neighbours that exist (the east zero of column nx adds nothing)
__device__ __forceinline__ double mgo_sum(const MgoLevel* L, int k, double pW, double pE, double pS, double pN) {
  const double tE = (k & 2) ? L->cx * pE : 0.0;
  const double tW = (k & 1) ? L->cx * pW : 0.0;
  const double tN = (k & 8) ? L->cy * pN : 0.0;
  const double tS = (k & 4) ? L->cy * pS : 0.0;
  return (tE + tW) + (tN + tS);
}

// Gauss-Seidel update of cell (j, i): rdiag (sum - f)
__device__ __forceinline__ double mgo_relax(const MgoLevel* L, int j, int i, double pW, double pE, double pS, double pN,
                                            double f) {
  const int k = mgo_mask(L, j, i);
  return L->rdiag[k] * (mgo_sum(L, k, pW, pE, pS, pN) - f);
}

// SOR update of the coarsest level: p (1 - w) + (w rdiag) (sum - f)
__device__ __forceinline__ double mgo_sor(const MgoLevel* L, int j, int i, double pc, double pW, double pE, double pS,
                                          double pN, double f) {
  const int k = mgo_mask(L, j, i);
  return pc * L->one_m_omega + L->omr[k] * (mgo_sum(L, k, pW, pE, pS, pN) - f);
}

// residual (cx (pE - c) + cx (pW - c)) + (cy (pN - c) + cy (pS - c)) - f; column nx: cE (0 - c) for its east term
__device__ __forceinline__ double mgo_resid(const MgoLevel* L, int j, int i, double c, double pW, double pE, double pS,
                                            double pN, double f) {
  const int k = mgo_mask(L, j, i);
  const double tE = (k & 2) ? L->cx * (pE - c) : L->cE * (0.0 - c);
  const double tW = (k & 1) ? L->cx * (pW - c) : 0.0;
  const double tN = (k & 8) ? L->cy * (pN - c) : 0.0;
  const double tS = (k & 4) ? L->cy * (pS - c) : 0.0;
  return ((tE + tW) + (tN + tS)) - f;
}

// residual of fine cell (j, i) from a field with rows of P doubles (global memory or LDS)
__device__ __forceinline__ double mgo_resid_at(const MgoLevel* Lf, const double* p, const double* f, size_t P, int j,
                                               int i) {
  const size_t o = (size_t)j * P + i;
  return mgo_resid(Lf, j, i, p[o], p[o - 1], p[o + 1], p[o - P], p[o + P], f[o]);
}

// Coarse source of cell (J, I): minus the mean of the residual over its children - four
// (-1/4 ((rSW + rSE) + (rNW + rNE))), or two along the halved direction (-1/2 (rW + rE), -1/2 (rS + rN)).
__device__ __forceinline__ double mgo_restrict_cell(const MgoLevel* Lf, const double* p, const double* f, size_t P, int J,
                                                    int I) {
  if (Lf->kind == MGO_X) {
    const double rW = mgo_resid_at(Lf, p, f, P, J, 2 * I - 1), rE = mgo_resid_at(Lf, p, f, P, J, 2 * I);
    return -0.5 * (rW + rE);
  }
  if (Lf->kind == MGO_Y) {
    const double rS = mgo_resid_at(Lf, p, f, P, 2 * J - 1, I), rN = mgo_resid_at(Lf, p, f, P, 2 * J, I);
    return -0.5 * (rS + rN);
  }
  const int j = 2 * J - 1, i = 2 * I - 1;
  const double rSW = mgo_resid_at(Lf, p, f, P, j, i), rSE = mgo_resid_at(Lf, p, f, P, j, i + 1);
  const double rNW = mgo_resid_at(Lf, p, f, P, j + 1, i), rNE = mgo_resid_at(Lf, p, f, P, j + 1, i + 1);
  return -0.25 * ((rSW + rSE) + (rNW + rNE));
}

// e of the coarse level with one ghost layer: south / north ghosts = rows 1 / ny, then
// the west ghost = column 1 and the east ghost = column nx times g (the line through the zero).
__device__ __forceinline__ double mgo_ext(const MgoLevel* Lc, const double* e, int pitch, int J, int I) {
  const int jj = min(max(J, 1), Lc->ny);
  if (I == 0) return e[(size_t)jj * pitch + 1];
  if (I == Lc->nx + 1) return e[(size_t)jj * pitch + Lc->nx] * Lc->g;
  return e[(size_t)jj * pitch + I];
}

// correction of fine cell (j, i): bilinear (((9 c + 3 V) + 3 H) + D) / 16, or linear along the
// halved direction, (3 c + H) / 4 or (3 c + V) / 4; V / H / D the coarse neighbours on the child's side
__device__ __forceinline__ double mgo_corr(const MgoLevel* Lc, int kind, const double* e, int pitch, int j, int i) {
  const int dj = (j & 1) ? -1 : 1, di = (i & 1) ? -1 : 1;
  if (kind == MGO_X) {
    const int I = (i + 1) >> 1;
    return (3.0 * e[(size_t)j * pitch + I] + mgo_ext(Lc, e, pitch, j, I + di)) * 0.25;
  }
  if (kind == MGO_Y) {
    const int J = (j + 1) >> 1;
    return (3.0 * e[(size_t)J * pitch + i] + mgo_ext(Lc, e, pitch, J + dj, i)) * 0.25;
  }
  const int J = (j + 1) >> 1, I = (i + 1) >> 1;
  const double c = e[(size_t)J * pitch + I];
  const double V = mgo_ext(Lc, e, pitch, J + dj, I);
  const double H = mgo_ext(Lc, e, pitch, J, I + di);
  const double D = mgo_ext(Lc, e, pitch, J + dj, I + di);
  return (((9.0 * c + 3.0 * V) + 3.0 * H) + D) * 0.0625;
}

struct MgChannel {
  using Level = MgoLevel;
  static constexpr bool has_pair = false;
  static constexpr bool pair_loads = true;
  static __device__ __forceinline__ bool unknown(const Level*, int, int) { return true; }
  static __device__ __forceinline__ double relax(const Level* L, int j, int i, double pW, double pE, double pS, double pN,
                                                 double f) {
    return mgo_relax(L, j, i, pW, pE, pS, pN, f);
  }
  static __device__ __forceinline__ double update(const Level* L, const double* p, int P, int j, int i, double f, bool sor) {
    return sor ? mgo_sor(L, j, i, p[0], p[-1], p[1], p[-P], p[P], f) : mgo_relax(L, j, i, p[-1], p[1], p[-P], p[P], f);
  }
  template <bool Aligned>
  static __device__ __forceinline__ double coarse_source(const Level* Lf, const double* p, const double* f, size_t P, int J,
                                                         int I) {
    return mgo_restrict_cell(Lf, p, f, P, J, I);
  }
  static __device__ __forceinline__ double corr(const Level* L, const double* e, int pitch, int j, int i) {
    return mgo_corr(L + 1, L->kind, e, pitch, j, i);
  }
};

// =============================================================== the step ==
// The third scheme (mg.hpp "the step", tests/mg_step_reference.py): the
// channel's operator over the fluid cells of the backwards-facing step. Two
// integer compares tell fluid from solid; a neighbour exists if it is inside
// the grid and fluid. The pair A = (jm+1, si+1), B = (jm, si) is coupled
// through the eliminated corner solid and has one colour ("the kernels").

__device__ __forceinline__ bool mgs_fluid(const MgsLevel* L, int j, int i) { return i > L->si || j <= L->jm; }
__device__ __forceinline__ bool mgs_is_a(const MgsLevel* L, int j, int i) { return j == L->jm + 1 && i == L->si + 1; }
__device__ __forceinline__ bool mgs_is_b(const MgsLevel* L, int j, int i) { return j == L->jm && i == L->si; }

// of a fluid cell (east and south of a fluid cell are fluid)
__device__ __forceinline__ int mgs_mask(const MgsLevel* L, int j, int i) {
  const int w = i > 1 && (i - 1 > L->si || j <= L->jm);
  const int n = j < L->ny && (i > L->si || j + 1 <= L->jm);
  return w | (int)(i < L->nx) << 1 | (int)(j > 1) << 2 | n << 3;
}

// The update of fluid cell (j, i), p pointing at it in a field with rows of P doubles (global memory or
// LDS): Gauss-Seidel rdiag (sum - f), or the coarsest level's SOR p (1 - w) + (w rdiag) (sum - f);
// sum = (cx pE + cx pW) + (cy pN + cy pS) over the neighbours that exist, with A's west term
// (cx/2) p_B and B's north term (cy/2) p_A.
__device__ __forceinline__ double mgs_update(const MgsLevel* L, const double* p, int P, int j, int i, double f, bool sor) {
  const int k = mgs_mask(L, j, i);
  const bool isa = mgs_is_a(L, j, i), isb = mgs_is_b(L, j, i);
  const double tE = (k & 2) ? L->cx * p[1] : 0.0;
  double tW = (k & 1) ? L->cx * p[-1] : 0.0;
  double tN = (k & 8) ? L->cy * p[P] : 0.0;
  const double tS = (k & 4) ? L->cy * p[-P] : 0.0;
  if (isa) tW = L->chx * p[-P - 1];
  if (isb) tN = L->chy * p[P + 1];
  const double s = ((tE + tW) + (tN + tS)) - f;
  if (sor) return p[0] * L->one_m_omega + (isa ? L->omrA : isb ? L->omrB : L->omr[k]) * s;
  return (isa ? L->rdA : isb ? L->rdB : L->rdiag[k]) * s;
}

// residual of fine cell (j, i): the channel's, 0 in a solid cell; A's west term (cx/2)(p_B - c), B's north (cy/2)(p_A - c)
__device__ __forceinline__ double mgs_resid_at(const MgsLevel* L, const double* p, const double* f, size_t P, int j,
                                               int i) {
  if (!mgs_fluid(L, j, i)) return 0.0;
  const size_t o = (size_t)j * P + i;
  const int k = mgs_mask(L, j, i);
  const double c = p[o];
  const double tE = (k & 2) ? L->cx * (p[o + 1] - c) : L->cE * (0.0 - c);
  double tW = (k & 1) ? L->cx * (p[o - 1] - c) : 0.0;
  double tN = (k & 8) ? L->cy * (p[o + P] - c) : 0.0;
  const double tS = (k & 4) ? L->cy * (p[o - P] - c) : 0.0;
  if (mgs_is_a(L, j, i)) tW = L->chx * (p[o - P - 1] - c);
  if (mgs_is_b(L, j, i)) tN = L->chy * (p[o + P + 1] - c);
  return ((tE + tW) + (tN + tS)) - f[o];
}

// Coarse source of cell (J, I) of level Lf + 1 (mgo_restrict_cell's three kinds); 0 in a solid coarse cell,
// whose children are all solid (a halved direction's block edge is even).
__device__ __forceinline__ double mgs_restrict_cell(const MgsLevel* Lf, const double* p, const double* f, size_t P, int J,
                                                    int I) {
  if (!mgs_fluid(Lf + 1, J, I)) return 0.0;
  if (Lf->kind == MGO_X) {
    const double rW = mgs_resid_at(Lf, p, f, P, J, 2 * I - 1), rE = mgs_resid_at(Lf, p, f, P, J, 2 * I);
    return -0.5 * (rW + rE);
  }
  if (Lf->kind == MGO_Y) {
    const double rS = mgs_resid_at(Lf, p, f, P, 2 * J - 1, I), rN = mgs_resid_at(Lf, p, f, P, 2 * J, I);
    return -0.5 * (rS + rN);
  }
  const int j = 2 * J - 1, i = 2 * I - 1;
  const double rSW = mgs_resid_at(Lf, p, f, P, j, i), rSE = mgs_resid_at(Lf, p, f, P, j, i + 1);
  const double rNW = mgs_resid_at(Lf, p, f, P, j + 1, i), rNE = mgs_resid_at(Lf, p, f, P, j + 1, i + 1);
  return -0.25 * ((rSW + rSE) + (rNW + rNE));
}

// inside the coarse grid and fluid
__device__ __forceinline__ bool mgs_present(const MgsLevel* Lc, int J, int I) {
  return J >= 1 && J <= Lc->ny && I >= 1 && I <= Lc->nx && mgs_fluid(Lc, J, I);
}

// correction of fluid fine cell (j, i): mgo_corr's formulas. A vertical or horizontal coarse neighbour
// that is missing (solid, or beyond a Neumann side) takes the centre value c, the east ghost c g; a
// missing diagonal the H value if V is missing, else the V value if H is missing, else c; an
// east-ghost diagonal V' g.
__device__ __forceinline__ double mgs_corr(const MgsLevel* Lc, int kind, const double* e, int pitch, int j, int i) {
  const int dj = kind == MGO_X ? 0 : (j & 1) ? -1 : 1, di = kind == MGO_Y ? 0 : (i & 1) ? -1 : 1;
  const int J = kind == MGO_X ? j : (j + 1) >> 1, I = kind == MGO_Y ? i : (i + 1) >> 1;
  const double c = e[(size_t)J * pitch + I];
  const bool Vp = mgs_present(Lc, J + dj, I);
  const double V = Vp ? e[(size_t)(J + dj) * pitch + I] : c;
  if (kind == MGO_Y) return (3.0 * c + V) * 0.25;
  const bool east = I + di == Lc->nx + 1;
  const bool Hp = mgs_present(Lc, J, I + di);
  const double H = east ? c * Lc->g : Hp ? e[(size_t)J * pitch + I + di] : c;
  if (kind == MGO_X) return (3.0 * c + H) * 0.25;
  double D;
  if (east) D = V * Lc->g;
  else if (mgs_present(Lc, J + dj, I + di)) D = e[(size_t)(J + dj) * pitch + I + di];
  else D = !Vp ? H : !Hp ? V : c;
  return (((9.0 * c + 3.0 * V) + 3.0 * H) + D) * 0.0625;
}

struct MgStep {
  using Level = MgsLevel;
  static constexpr bool has_pair = true;     // A's thread writes A and B, B's own writes nothing
  static constexpr bool pair_loads = false;  // the pair's diagonal neighbours: scalar loads around the cell
  static __device__ __forceinline__ bool unknown(const Level* L, int j, int i) { return mgs_fluid(L, j, i); }
  static __device__ __forceinline__ bool is_a(const Level* L, int j, int i) { return mgs_is_a(L, j, i); }
  static __device__ __forceinline__ bool is_b(const Level* L, int j, int i) { return mgs_is_b(L, j, i); }
  static __device__ __forceinline__ double update(const Level* L, const double* p, int P, int j, int i, double f, bool sor) {
    return mgs_update(L, p, P, j, i, f, sor);
  }
  template <bool Aligned>
  static __device__ __forceinline__ double coarse_source(const Level* Lf, const double* p, const double* f, size_t P, int J,
                                                         int I) {
    return mgs_restrict_cell(Lf, p, f, P, J, I);
  }
  static __device__ __forceinline__ double corr(const Level* L, const double* e, int pitch, int j, int i) {
    return mgs_corr(L + 1, L->kind, e, pitch, j, i);
  }
};

// =================================================== the cavity, any size ==
// The fourth scheme (mg.hpp "the cavity at any size", tests/mg_any_reference.py):
// the cavity's operator with the coefficients of the face between a direction's
// last two cells, and the transfers' weights at a direction's end. A cell whose
// stencil touches no such face takes the cavity's expressions (a coefficient of
// 1 is not multiplied with: the same bits); a coarse cell or a fine cell that
// takes none of the weights takes the cavity's transfer.

__device__ __forceinline__ bool mga_plain(const MgaLevel* L, int j, int i) {
  return i > 1 && i < L->x.lim && j > 1 && j < L->y.lim;
}

__device__ __forceinline__ MgCoef mga_coef(const MgaLevel* L, int j, int i) {
  MgCoef k;
  const int cx = i == 1 ? 0 : i == L->nx ? 3 : i == L->nx - 1 ? 2 : 1;
  const int cy = j == 1 ? 0 : j == L->ny ? 3 : j == L->ny - 1 ? 2 : 1;
  k.ew = cx == 0 ? 0.0 : cx == 3 ? L->x.c_hi : 1.0;
  k.ee = cx == 3 ? 0.0 : cx == 2 ? L->x.c_lo : 1.0;
  k.cs = cy == 0 ? L->cS : cy == 3 ? L->y.c_hi : 1.0;
  k.en = cy == 3 ? 0.0 : cy == 2 ? L->y.c_lo : 1.0;
  k.idx = cx | cy << 2;
  return k;
}

__device__ __forceinline__ double mga_relax(const MgaLevel* L, int j, int i, double pW, double pE, double pS, double pN,
                                            double f) {
  if (mga_plain(L, j, i)) return L->rdiag[5] * (((pE + pW) + (pN + pS)) - f * L->h2);
  const MgCoef k = mga_coef(L, j, i);
  return L->rdiag[k.idx] * (((k.ee * pE + k.ew * pW) + (k.en * pN + k.cs * pS)) - f * L->h2);
}

__device__ __forceinline__ double mga_sor(const MgaLevel* L, int j, int i, double pc, double pW, double pE, double pS,
                                          double pN, double f) {
  const MgCoef k = mga_coef(L, j, i);
  return pc * L->one_m_omega + L->omr[k.idx] * (((k.ee * pE + k.ew * pW) + (k.en * pN + k.cs * pS)) - f * L->h2);
}

__device__ __forceinline__ double mga_resid(const MgaLevel* L, int j, int i, double c, double pW, double pE, double pS,
                                            double pN, double f) {
  if (mga_plain(L, j, i)) return L->ih2 * ((((pE - c) + (pW - c)) + (pN - c)) + (pS - c)) - f;
  const MgCoef k = mga_coef(L, j, i);
  return L->ih2 * (((k.ee * (pE - c) + k.ew * (pW - c)) + k.en * (pN - c)) + k.cs * (pS - c)) - f;
}

// residual of fine cell (j, i), 1 <= j <= ny and 1 <= i <= nx, from fields with rows of P doubles
__device__ __forceinline__ double mga_resid_at(const MgaLevel* Lf, const double* p, const double* f, size_t P, int j,
                                               int i) {
  const size_t o = (size_t)j * P + i;
  return mga_resid(Lf, j, i, p[o], p[o - 1], p[o + 1], p[o - P], p[o + P], f[o]);
}

// Coarse source of a cell in the last coarse column of an irregular x and / or the last coarse row of an
// irregular y: -(b0 hS + b1 hN), hS = a0 rSW + a1 rSE and hN alike; a direction's single child stands alone.
// Only children inside the grid are read.
__device__ __forceinline__ double mga_restrict_edge(const MgaLevel* Lf, const double* p, const double* f, size_t P, int J,
                                                    int I, bool lx, bool ly) {
  const int j = 2 * J - 1, i = 2 * I - 1;
  const bool sx = lx && Lf->x.single, sy = ly && Lf->y.single;
  const double a0 = lx ? Lf->x.r0 : 0.5, a1 = lx ? Lf->x.r1 : 0.5;
  const double b0 = ly ? Lf->y.r0 : 0.5, b1 = ly ? Lf->y.r1 : 0.5;
  double hS = mga_resid_at(Lf, p, f, P, j, i);
  if (!sx) hS = a0 * hS + a1 * mga_resid_at(Lf, p, f, P, j, i + 1);
  if (sy) return -hS;
  double hN = mga_resid_at(Lf, p, f, P, j + 1, i);
  if (!sx) hN = a0 * hN + a1 * mga_resid_at(Lf, p, f, P, j + 1, i + 1);
  return -(b0 * hS + b1 * hN);
}

// correction of fine cell (j, i): the cavity's, but where i >= x.first or j >= y.first:
// ay (ax c + bx H) + by (ax V + bx D) with the directions' weights (3/4, 1/4 in a regular one); b = 0 drops its terms
__device__ __forceinline__ double mga_corr(const MgaLevel* L, const double* e, int pitch, int j, int i) {
  const MgLevel* Lc = L + 1;
  const int kx = i - L->x.first, ky = j - L->y.first;
  if (kx < 0 && ky < 0) return mg_corr(Lc, e, pitch, j, i);
  const double ax = kx < 0 ? 0.75 : L->x.pa[kx], bx = kx < 0 ? 0.25 : L->x.pb[kx];
  const double ay = ky < 0 ? 0.75 : L->y.pa[ky], by = ky < 0 ? 0.25 : L->y.pb[ky];
  const int J = (j + 1) >> 1, I = (i + 1) >> 1;
  const int dj = (j & 1) ? -1 : 1, di = (i & 1) ? -1 : 1;
  double rc = e[(size_t)J * pitch + I];
  if (bx != 0.0) rc = ax * rc + bx * mg_ext(Lc, e, pitch, J, I + di);
  if (by == 0.0) return rc;
  double rv = mg_ext(Lc, e, pitch, J + dj, I);
  if (bx != 0.0) rv = ax * rv + bx * mg_ext(Lc, e, pitch, J + dj, I + di);
  return ay * rc + by * rv;
}

struct MgAny {
  using Level = MgaLevel;
  static constexpr bool has_pair = false;
  static constexpr bool pair_loads = true;
  static __device__ __forceinline__ bool unknown(const Level*, int, int) { return true; }
  static __device__ __forceinline__ double relax(const Level* L, int j, int i, double pW, double pE, double pS, double pN,
                                                 double f) {
    return mga_relax(L, j, i, pW, pE, pS, pN, f);
  }
  static __device__ __forceinline__ double update(const Level* L, const double* p, int P, int j, int i, double f, bool sor) {
    return sor ? mga_sor(L, j, i, p[0], p[-1], p[1], p[-P], p[P], f) : mga_relax(L, j, i, p[-1], p[1], p[-P], p[P], f);
  }
  // An edge cell (above) reads its children cell by cell; every other coarse cell has four children inside
  // the grid and is the cavity's: the 4 x 4 block p(2J-2 .. 2J+1, 2I-2 .. 2I+1), 2I+1 <= nx+1 and 2J+1 <= ny+1.
  template <bool Aligned>
  static __device__ __forceinline__ double coarse_source(const Level* Lf, const double* p, const double* f, size_t P, int J,
                                                         int I) {
    const bool lx = I == Lf->x.last, ly = J == Lf->y.last;
    if (lx || ly) return mga_restrict_edge(Lf, p, f, P, J, I, lx, ly);
    const size_t o = (size_t)(2 * J - 2) * P + (size_t)(2 * I - 2);
    double a[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (Aligned) {
        const double2 lo = *reinterpret_cast<const double2*>(p + o + r * P);
        const double2 hi = *reinterpret_cast<const double2*>(p + o + r * P + 2);
        a[r][0] = lo.x, a[r][1] = lo.y, a[r][2] = hi.x, a[r][3] = hi.y;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) a[r][c] = p[o + r * P + c];
      }
    }
    const int j = 2 * J - 1, i = 2 * I - 1;
    const double rSW = mga_resid(Lf, j, i, a[1][1], a[1][0], a[1][2], a[0][1], a[2][1], f[o + P + 1]);
    const double rSE = mga_resid(Lf, j, i + 1, a[1][2], a[1][1], a[1][3], a[0][2], a[2][2], f[o + P + 2]);
    const double rNW = mga_resid(Lf, j + 1, i, a[2][1], a[2][0], a[2][2], a[1][1], a[3][1], f[o + 2 * P + 1]);
    const double rNE = mga_resid(Lf, j + 1, i + 1, a[2][2], a[2][1], a[2][3], a[1][2], a[3][2], f[o + 2 * P + 2]);
    return -0.25 * ((rSW + rSE) + (rNW + rNE));
  }
  static __device__ __forceinline__ double corr(const Level* L, const double* e, int pitch, int j, int i) {
    return mga_corr(L, e, pitch, j, i);
  }
};

// ================================================== the channel, any size ==
// The fifth scheme (mg.hpp "the channel at any size", tests/mg_open_any_reference.py):
// the channel's operator with the coefficients of the face between a direction's
// last two cells and of column nx's east zero, and the transfers' weights at a
// halved direction's end. A plain cell - west, east, south and north all with
// the level's cx / cy - is told by four compares against the level's x.lim /
// y.lim (the irregular flag is folded into them) and takes the channel's
// expressions without a class or a select; a coarse cell or a fine cell that
// takes none of the weights takes the channel's transfer.

__device__ __forceinline__ bool mgoa_plain(const MgoaLevel* L, int j, int i) {
  return i > 1 && i < L->x.lim && j > 1 && j < L->y.lim;
}

// the classes of a cell that is not plain, and the sum's terms over the neighbours that exist
struct MgoaCell {
  int kx, ky;
  double cw, ce, cs, cn;
};
__device__ __forceinline__ MgoaCell mgoa_cell(const MgoaLevel* L, int j, int i) {
  MgoaCell k;
  k.kx = i == 1 ? 0 : i == L->nx ? 3 : i == L->nx - 1 ? 2 : 1;
  k.ky = j == 1 ? 0 : j == L->ny ? 3 : j == L->ny - 1 ? 2 : 1;
  k.cw = k.kx == 3 ? L->x.c_hi : L->cx;
  k.ce = k.kx == 2 ? L->x.c_lo : L->cx;
  k.cs = k.ky == 3 ? L->y.c_hi : L->cy;
  k.cn = k.ky == 2 ? L->y.c_lo : L->cy;
  return k;
}

// (ce pE + cw pW) + (cn pN + cs pS) over the neighbours that exist (the east zero of column nx adds nothing)
__device__ __forceinline__ double mgoa_sum(const MgoaCell& k, double pW, double pE, double pS, double pN) {
  const double tE = k.kx != 3 ? k.ce * pE : 0.0;
  const double tW = k.kx != 0 ? k.cw * pW : 0.0;
  const double tN = k.ky != 3 ? k.cn * pN : 0.0;
  const double tS = k.ky != 0 ? k.cs * pS : 0.0;
  return (tE + tW) + (tN + tS);
}

__device__ __forceinline__ double mgoa_relax(const MgoaLevel* L, int j, int i, double pW, double pE, double pS, double pN,
                                             double f) {
  if (mgoa_plain(L, j, i)) return L->rdiag[5] * (((L->cx * pE + L->cx * pW) + (L->cy * pN + L->cy * pS)) - f);
  const MgoaCell k = mgoa_cell(L, j, i);
  return L->rdiag[k.kx | k.ky << 2] * (mgoa_sum(k, pW, pE, pS, pN) - f);
}

__device__ __forceinline__ double mgoa_sor(const MgoaLevel* L, int j, int i, double pc, double pW, double pE, double pS,
                                           double pN, double f) {
  const MgoaCell k = mgoa_cell(L, j, i);
  return pc * L->one_m_omega + L->omr[k.kx | k.ky << 2] * (mgoa_sum(k, pW, pE, pS, pN) - f);
}

// residual of fine cell (j, i), 1 <= j <= ny and 1 <= i <= nx, from fields with rows of P doubles:
// (ce (pE - c) + cw (pW - c)) + (cn (pN - c) + cs (pS - c)) - f; column nx: cE (0 - c) for its east term
__device__ __forceinline__ double mgoa_resid_at(const MgoaLevel* L, const double* p, const double* f, size_t P, int j,
                                                int i) {
  const size_t o = (size_t)j * P + i;
  const double c = p[o], pW = p[o - 1], pE = p[o + 1], pS = p[o - P], pN = p[o + P];
  if (mgoa_plain(L, j, i)) return ((L->cx * (pE - c) + L->cx * (pW - c)) + (L->cy * (pN - c) + L->cy * (pS - c))) - f[o];
  const MgoaCell k = mgoa_cell(L, j, i);
  const double tE = k.kx != 3 ? k.ce * (pE - c) : L->cE * (0.0 - c);
  const double tW = k.kx != 0 ? k.cw * (pW - c) : 0.0;
  const double tN = k.ky != 3 ? k.cn * (pN - c) : 0.0;
  const double tS = k.ky != 0 ? k.cs * (pS - c) : 0.0;
  return ((tE + tW) + (tN + tS)) - f[o];
}

// Coarse source of cell (J, I): the channel's three kinds; a cell in the last coarse column of an irregular
// halved x and / or the last coarse row of an irregular halved y: -(b0 hS + b1 hN), hS = a0 rSW + a1 rSE and
// hN alike, where a direction's single child, and a direction the transfer does not halve, stand alone.
// Only children inside the grid are read.
__device__ __forceinline__ double mgoa_restrict_cell(const MgoaLevel* Lf, const double* p, const double* f, size_t P, int J,
                                                     int I) {
  const int kind = Lf->kind;
  const bool lx = I == Lf->x.last, ly = J == Lf->y.last;  // (last 0: no such cell)
  if (lx || ly) {
    const int j = kind == MGO_X ? J : 2 * J - 1, i = kind == MGO_Y ? I : 2 * I - 1;
    const bool sx = kind == MGO_Y || (lx && Lf->x.single), sy = kind == MGO_X || (ly && Lf->y.single);
    const double a0 = lx ? Lf->x.r0 : 0.5, a1 = lx ? Lf->x.r1 : 0.5;
    const double b0 = ly ? Lf->y.r0 : 0.5, b1 = ly ? Lf->y.r1 : 0.5;
    double hS = mgoa_resid_at(Lf, p, f, P, j, i);
    if (!sx) hS = a0 * hS + a1 * mgoa_resid_at(Lf, p, f, P, j, i + 1);
    if (sy) return -hS;
    double hN = mgoa_resid_at(Lf, p, f, P, j + 1, i);
    if (!sx) hN = a0 * hN + a1 * mgoa_resid_at(Lf, p, f, P, j + 1, i + 1);
    return -(b0 * hS + b1 * hN);
  }
  if (kind == MGO_X) {
    const double rW = mgoa_resid_at(Lf, p, f, P, J, 2 * I - 1), rE = mgoa_resid_at(Lf, p, f, P, J, 2 * I);
    return -0.5 * (rW + rE);
  }
  if (kind == MGO_Y) {
    const double rS = mgoa_resid_at(Lf, p, f, P, 2 * J - 1, I), rN = mgoa_resid_at(Lf, p, f, P, 2 * J, I);
    return -0.5 * (rS + rN);
  }
  const int j = 2 * J - 1, i = 2 * I - 1;
  const double rSW = mgoa_resid_at(Lf, p, f, P, j, i), rSE = mgoa_resid_at(Lf, p, f, P, j, i + 1);
  const double rNW = mgoa_resid_at(Lf, p, f, P, j + 1, i), rNE = mgoa_resid_at(Lf, p, f, P, j + 1, i + 1);
  return -0.25 * ((rSW + rSE) + (rNW + rNE));
}

// correction of fine cell (j, i): the channel's, but where i >= x.first or j >= y.first (n + 1 in a direction
// that is regular or not halved): ay (ax c + bx H) + by (ax V + bx D) for a full transfer, ax c + bx H or
// ay c + by V along the one halved direction, with the directions' weights (3/4, 1/4 in a regular one); b = 0
// drops its term and leaves a times the other. The neighbours come through the channel's ghost layer.
__device__ __forceinline__ double mgoa_corr(const MgoaLevel* L, const double* e, int pitch, int j, int i) {
  const MgoLevel* Lc = L + 1;
  const int kind = L->kind;
  const int kx = i - L->x.first, ky = j - L->y.first;
  if (kx < 0 && ky < 0) return mgo_corr(Lc, kind, e, pitch, j, i);
  const double ax = kx < 0 ? 0.75 : L->x.pa[kx], bx = kx < 0 ? 0.25 : L->x.pb[kx];
  const double ay = ky < 0 ? 0.75 : L->y.pa[ky], by = ky < 0 ? 0.25 : L->y.pb[ky];
  const int J = kind == MGO_X ? j : (j + 1) >> 1, I = kind == MGO_Y ? i : (i + 1) >> 1;
  const int dj = (j & 1) ? -1 : 1, di = (i & 1) ? -1 : 1;
  const double c = e[(size_t)J * pitch + I];
  if (kind == MGO_X) return bx != 0.0 ? ax * c + bx * mgo_ext(Lc, e, pitch, J, I + di) : ax * c;
  if (kind == MGO_Y) return by != 0.0 ? ay * c + by * mgo_ext(Lc, e, pitch, J + dj, I) : ay * c;
  const double rc = bx != 0.0 ? ax * c + bx * mgo_ext(Lc, e, pitch, J, I + di) : ax * c;
  if (by == 0.0) return ay * rc;
  const double V = mgo_ext(Lc, e, pitch, J + dj, I);
  const double rv = bx != 0.0 ? ax * V + bx * mgo_ext(Lc, e, pitch, J + dj, I + di) : ax * V;
  return ay * rc + by * rv;
}

struct MgChannelAny {
  using Level = MgoaLevel;
  static constexpr bool has_pair = false;
  static constexpr bool pair_loads = true;
  static __device__ __forceinline__ bool unknown(const Level*, int, int) { return true; }
  static __device__ __forceinline__ double relax(const Level* L, int j, int i, double pW, double pE, double pS, double pN,
                                                 double f) {
    return mgoa_relax(L, j, i, pW, pE, pS, pN, f);
  }
  static __device__ __forceinline__ double update(const Level* L, const double* p, int P, int j, int i, double f, bool sor) {
    return sor ? mgoa_sor(L, j, i, p[0], p[-1], p[1], p[-P], p[P], f) : mgoa_relax(L, j, i, p[-1], p[1], p[-P], p[P], f);
  }
  template <bool Aligned>
  static __device__ __forceinline__ double coarse_source(const Level* Lf, const double* p, const double* f, size_t P, int J,
                                                         int I) {
    return mgoa_restrict_cell(Lf, p, f, P, J, I);
  }
  static __device__ __forceinline__ double corr(const Level* L, const double* e, int pitch, int j, int i) {
    return mgoa_corr(L, e, pitch, j, i);
  }
};

template <class Level> struct MgSchemeOf;
template <> struct MgSchemeOf<MgLevel> { using type = MgCavity; };
template <> struct MgSchemeOf<MgoLevel> { using type = MgChannel; };
template <> struct MgSchemeOf<MgsLevel> { using type = MgStep; };
template <> struct MgSchemeOf<MgaLevel> { using type = MgAny; };
template <> struct MgSchemeOf<MgoaLevel> { using type = MgChannelAny; };

// ============================================================ the kernels ==

// A coupled pair A = (jm+1, si+1), B = (jm, si) has one colour: wherever a colour is updated (the colour
// launch, the tile, the tail's half sweep), the thread that owns A forms both new values from the values of
// before the phase and writes both, and the thread that owns B writes nothing - no thread reads a cell
// another one writes in the same phase.

// ------------------------------------------------------ multi-launch levels --

// One colour of a sweep of level l, in place. Block: 4 waves = 4 rows x 128 columns, a lane the column pair
// (gi, gi + 1) and in it the colour's cell.
template <class S>
__global__ __launch_bounds__(256) void mg_smooth_kernel(const typename S::Level* __restrict__ lv, int l, double* p,
                                                        const double* __restrict__ f, int colour) {
  const typename S::Level* L = lv + l;
  const int nx = L->nx, ny = L->ny;
  const int gi = blockIdx.x * 128 + 2 * (threadIdx.x & 63);  // even: a 16-B aligned pair
  const int j = 1 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j > ny || gi > nx) return;
  const int t = (j + colour) & 1;  // colour 0 holds the cells with i + j even: component t of the pair
  const int i = gi + t;
  if (i < 1 || i > nx) return;
  if constexpr (S::pair_loads) {
    static_assert(!S::has_pair, "the pair's diagonal neighbours are not in the aligned loads");
    const size_t P = (size_t)L->pitch, o = (size_t)j * P + gi;
    const double2 pc = *reinterpret_cast<const double2*>(p + o);
    const double2 ps = *reinterpret_cast<const double2*>(p + o - P);
    const double2 pn = *reinterpret_cast<const double2*>(p + o + P);
    const double2 fc = *reinterpret_cast<const double2*>(f + o);
    double v;
    if (t == 0) v = S::relax(L, j, i, p[o - 1], pc.y, ps.x, pn.x, fc.x);  // (i >= 2: o - 1 is column i - 1 >= 1)
    else v = S::relax(L, j, i, pc.x, p[o + 2], ps.y, pn.y, fc.y);        // (o + 2: column i + 1 <= nx + 1 < pitch)
    p[o + t] = v;
  } else {
    if (!S::unknown(L, j, i)) return;
    if constexpr (S::has_pair) {
      if (S::is_b(L, j, i)) return;
    }
    const int P = L->pitch;
    const size_t o = (size_t)j * P + i;
    const double v = S::update(L, p + o, P, j, i, f[o], false);
    if constexpr (S::has_pair) {
      if (S::is_a(L, j, i)) {  // both from the values of before the launch
        const size_t ob = o - P - 1;
        const double vb = S::update(L, p + ob, P, j - 1, i - 1, f[ob], false);
        p[ob] = vb;
      }
    }
    p[o] = v;
  }
}

// nsw (1..3) whole sweeps of level l in one launch, pin -> pout (as tile.hip
// does for SOR). A workgroup of 16 waves holds a region of MG_TR rows x 128
// columns of p in LDS: its tile plus H = 2 nsw cells of halo on every side,
// since each colour phase leaves one more ring next to the region's border
// stale. Phase k (colour k & 1 of sweep k >> 1) updates the cells at least
// k + 1 from the border; after 2 nsw phases the tile itself (margin H) holds
// what the sweeps over the whole level give - the halo cells are recomputed by
// the neighbouring workgroups, same operands, same bits. p and f are read
// once (1.2x with the halos) and p written once: 24-28 B per cell for nsw
// sweeps where the colour launches move up to 48 per sweep. Lane l owns the
// aligned column pair (2l, 2l + 1) of rows w, w + 16, ... and keeps their f
// in registers; region column c is global column bx TW - H + c (even offset:
// the pairs stay 16-B aligned), region row r global row by TH - H + r. Cells
// outside rows 0 .. ny+1 / columns 0 .. nx+1 are loaded as 0. Only unknowns
// are updated and written. A coupled pair is a diagonal dependency (Chebyshev
// distance 1): the halo's shrink of one cell per phase holds for it.
template <class S>
__global__ __launch_bounds__(MG_TILE_THREADS) void mg_smooth_tile_kernel(const typename S::Level* __restrict__ lv, int l,
                                                                         const double* __restrict__ pin,
                                                                         double* __restrict__ pout,
                                                                         const double* __restrict__ f, int nsw) {
  __shared__ double T[MG_TR * MG_TC];
  const typename S::Level* L = lv + l;
  const int nx = L->nx, ny = L->ny;
  const int H = 2 * nsw, TW = MG_TC - 2 * H, TH = MG_TR - 2 * H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = 2 * lane;
  const int gx = (int)blockIdx.x * TW - H + c0;  // even (or negative: outside)
  const int gy0 = (int)blockIdx.y * TH - H;
  const size_t P = (size_t)L->pitch;
  const bool colin = gx >= 0 && gx <= nx + 1;  // (gx + 1 <= nx + 2 < pitch)
  double2 fr[MG_TQ];
#pragma unroll
  for (int q = 0; q < MG_TQ; ++q) {
    const int r = w + 16 * q, gy = gy0 + r;
    double2 v = make_double2(0.0, 0.0);
    fr[q] = v;
    if (colin && gy >= 0 && gy <= ny + 1) {
      v = *reinterpret_cast<const double2*>(pin + (size_t)gy * P + gx);
      fr[q] = *reinterpret_cast<const double2*>(f + (size_t)gy * P + gx);
    }
    *reinterpret_cast<double2*>(&T[r * MG_TC + c0]) = v;
  }
  __syncthreads();
  for (int k = 0; k < 2 * nsw; ++k) {
#pragma unroll
    for (int q = 0; q < MG_TQ; ++q) {
      const int r = w + 16 * q, gy = gy0 + r;
      const int t = (gy + k) & 1;  // colour k & 1: the cells with i + j + colour even (gx is even)
      const int c = c0 + t, i = gx + t;
      const int o = r * MG_TC + c;
      const bool own = r > k && r < MG_TR - 1 - k && c > k && c < MG_TC - 1 - k;
      const bool cell = gy >= 1 && gy <= ny && i >= 1 && i <= nx;
      if constexpr (S::has_pair) {
        if (!cell || !S::unknown(L, gy, i) || S::is_b(L, gy, i)) continue;
        // B = (r - 1, c - 1) by A's thread, under B's own condition (then A, at least k from the border, holds
        // its value of before the phase; r - 1 > k >= 0 and c - 1 > k keep the cell and its neighbours inside)
        const bool pair = S::is_a(L, gy, i) && r - 1 > k && r - 1 < MG_TR - 1 - k && c - 1 > k && c - 1 < MG_TC - 1 - k;
        double v = 0.0, vb = 0.0;
        if (own) v = S::update(L, T + o, MG_TC, gy, i, t ? fr[q].y : fr[q].x, false);
        if (pair) vb = S::update(L, T + o - MG_TC - 1, MG_TC, gy - 1, i - 1, f[(size_t)(gy - 1) * P + (i - 1)], false);
        if (own) T[o] = v;
        if (pair) T[o - MG_TC - 1] = vb;
      } else {
        if (own && cell) T[o] = S::update(L, T + o, MG_TC, gy, i, t ? fr[q].y : fr[q].x, false);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < MG_TQ; ++q) {
    const int r = w + 16 * q, gy = gy0 + r;
    if (r < H || r >= H + TH || c0 < H || c0 >= H + TW || gy < 1 || gy > ny) continue;  // (H, TW even: a pair is owned whole)
    const double2 v = *reinterpret_cast<const double2*>(&T[r * MG_TC + c0]);
    double* o = pout + (size_t)gy * P + gx;
    const bool wa = gx >= 1 && gx <= nx && S::unknown(L, gy, gx), wb = gx + 1 >= 1 && gx + 1 <= nx && S::unknown(L, gy, gx + 1);
    if (wa && wb) *reinterpret_cast<double2*>(o) = v;
    else if (wa) o[0] = v.x;
    else if (wb) o[1] = v.y;
  }
}

// Residual of level l + restriction to level l + 1 (full weighting, or over the two children along the
// direction level l halves); e_{l+1} = 0. One thread per coarse cell; block: 4 coarse rows x 64 coarse columns.
template <class S>
__global__ __launch_bounds__(256) void mg_restrict_kernel(const typename S::Level* __restrict__ lv, int l,
                                                          const double* __restrict__ p, const double* __restrict__ f,
                                                          double* __restrict__ fc, double* __restrict__ ec) {
  const typename S::Level* Lf = lv + l;
  const typename S::Level* Lc = lv + l + 1;
  const int I = 1 + blockIdx.x * 64 + (threadIdx.x & 63);
  const int J = 1 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (I > Lc->nx || J > Lc->ny) return;
  const size_t oc = (size_t)J * Lc->pitch + I;
  fc[oc] = S::template coarse_source<true>(Lf, p, f, (size_t)Lf->pitch, J, I);
  ec[oc] = 0.0;
}

// p_l += interpolant of e_{l+1} on the unknowns. Block: 4 rows x 128 columns, a lane one aligned pair.
template <class S>
__global__ __launch_bounds__(256) void mg_prolong_kernel(const typename S::Level* __restrict__ lv, int l,
                                                         double* __restrict__ p, const double* __restrict__ ec) {
  const typename S::Level* L = lv + l;
  const int nx = L->nx, ny = L->ny;
  const int gi = blockIdx.x * 128 + 2 * (threadIdx.x & 63);
  const int j = 1 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j > ny || gi > nx) return;
  const size_t o = (size_t)j * L->pitch + gi;
  const int pc = (L + 1)->pitch;
  const bool wa = gi >= 1 && S::unknown(L, j, gi), wb = gi + 1 <= nx && S::unknown(L, j, gi + 1);  // (nx >= 2)
  if (wa && wb) {
    double2 v = *reinterpret_cast<const double2*>(p + o);
    v.x += S::corr(L, ec, pc, j, gi);
    v.y += S::corr(L, ec, pc, j, gi + 1);
    *reinterpret_cast<double2*>(p + o) = v;
  } else if (wa) {
    p[o] += S::corr(L, ec, pc, j, gi);  // (gi == nx, or its east neighbour is no unknown)
  } else if (wb) {
    p[o + 1] += S::corr(L, ec, pc, j, gi + 1);  // (gi == 0, or gi is no unknown)
  }
}

// ------------------------------------------------------- one-launch tail --

// one colour of a sweep of a level held in LDS (rows of nx + 2), by the whole workgroup
template <class S>
__device__ __forceinline__ void mg_tail_half_sweep(const typename S::Level* L, double* p, const double* f, int colour,
                                                   bool sor) {
  const int nx = L->nx, ny = L->ny, pitch = nx + 2, hw = (nx + 1) >> 1;
  for (int q = threadIdx.x; q < ny * hw; q += MG_TAIL_THREADS) {
    const int j = 1 + q / hw;
    const int i = 1 + ((j + 1 + colour) & 1) + 2 * (q % hw);
    if (i > nx || !S::unknown(L, j, i)) continue;
    if constexpr (S::has_pair) {
      if (S::is_b(L, j, i)) continue;
    }
    const int o = j * pitch + i;
    const double v = S::update(L, p + o, pitch, j, i, f[o], sor);
    if constexpr (S::has_pair) {
      if (S::is_a(L, j, i)) {
        const int ob = o - pitch - 1;
        const double vb = S::update(L, p + ob, pitch, j - 1, i - 1, f[ob], sor);
        p[ob] = vb;
      }
    }
    p[o] = v;
  }
  __syncthreads();
}

// The sub-cycle over levels l0 .. last in one workgroup, each transfer by its fine level.
template <class S>
__global__ __launch_bounds__(MG_TAIL_THREADS) void mg_tail_kernel(const typename S::Level* __restrict__ lv, int l0,
                                                                  int last, int nu1, int nu2,
                                                                  const double* __restrict__ fg, double* __restrict__ eg) {
  using Level = typename S::Level;
  __shared__ double T[MG_LDS_DOUBLES];
  const int tid = threadIdx.x;
  // every level's correction starts from zero, ghosts (and cells that are no unknowns) included
  for (int l = l0; l <= last; ++l) {
    const Level* L = lv + l;
    const int n = (L->nx + 2) * (L->ny + 2);
    for (int q = tid; q < n; q += MG_TAIL_THREADS) T[L->lds_p + q] = 0.0;
  }
  {
    const Level* L = lv + l0;
    const int nx = L->nx;
    for (int q = tid; q < nx * L->ny; q += MG_TAIL_THREADS) {
      const int j = 1 + q / nx, i = 1 + q % nx;
      T[L->lds_f + j * (nx + 2) + i] = fg[(size_t)j * L->pitch + i];
    }
  }
  __syncthreads();
  for (int l = l0; l < last; ++l) {
    const Level* L = lv + l;
    const Level* Lc = L + 1;
    double* p = T + L->lds_p;
    const double* f = T + L->lds_f;
    for (int s = 0; s < nu1; ++s) {
      mg_tail_half_sweep<S>(L, p, f, 0, false);
      mg_tail_half_sweep<S>(L, p, f, 1, false);
    }
    const int ncx = Lc->nx, pcp = ncx + 2;
    for (int q = tid; q < ncx * Lc->ny; q += MG_TAIL_THREADS) {
      const int J = 1 + q / ncx, I = 1 + q % ncx;
      T[Lc->lds_f + J * pcp + I] = S::template coarse_source<false>(L, p, f, (size_t)(L->nx + 2), J, I);
    }
    __syncthreads();
  }
  {
    const Level* L = lv + last;
    double* p = T + L->lds_p;
    const double* f = T + L->lds_f;
    for (int s = 0; s < L->coarse_sweeps; ++s) {
      mg_tail_half_sweep<S>(L, p, f, 0, true);
      mg_tail_half_sweep<S>(L, p, f, 1, true);
    }
  }
  for (int l = last - 1; l >= l0; --l) {
    const Level* L = lv + l;
    double* p = T + L->lds_p;
    const double* f = T + L->lds_f;
    const double* e = T + (L + 1)->lds_p;
    const int nx = L->nx, pf = nx + 2, pe = (L + 1)->nx + 2;
    for (int q = tid; q < nx * L->ny; q += MG_TAIL_THREADS) {
      const int j = 1 + q / nx, i = 1 + q % nx;
      if (S::unknown(L, j, i)) p[j * pf + i] += S::corr(L, e, pe, j, i);
    }
    __syncthreads();
    for (int s = 0; s < nu2; ++s) {
      mg_tail_half_sweep<S>(L, p, f, 0, false);
      mg_tail_half_sweep<S>(L, p, f, 1, false);
    }
  }
  {
    const Level* L = lv + l0;
    const int nx = L->nx;
    for (int q = tid; q < nx * L->ny; q += MG_TAIL_THREADS) {
      const int j = 1 + q / nx, i = 1 + q % nx;
      eg[(size_t)j * L->pitch + i] = T[L->lds_p + j * (nx + 2) + i];
    }
  }
}

// ---------------------------------------------------------- the step only --


// The reference's ghost and solid refresh of level 0 (mg.hpp: mgs_refresh_launch). Thread t serves row t
// (its west and east ghosts, its face-column cell) and column t (its south and north ghosts, its face-row
// cell, the corner). The two ghosts that copy a face cell take its value of before this refresh, as the
// reference's order gives it (ghost sides first): the thread that reads it from prev is the one that
// then writes the cell in cur. The block is at least 2 columns wide and 2 rows high (the geometry rule).
__global__ __launch_bounds__(256) void mgs_refresh_kernel(int nx, int ny, int P, int si, int jm, double* cur,
                                                          const double* prev, const double* own) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int jb = jm + 1;
  if (t >= 1 && t <= ny) {
    const size_t o = (size_t)t * P;
    cur[o] = t <= jm ? cur[o + 1] : t == jb ? prev[o + 1] : own[o + 1];
    cur[o + nx + 1] = 0.0;
    if (t == jb) cur[o + 1] = 0.0 + cur[o - P + 1];             // face row, column 1 (after its old value went west)
    if (t > jb && t < ny) cur[o + si] = 0.0 + cur[o + si + 1];  // face column (row ny: by column si's thread)
  }
  if (t >= 1 && t <= nx) {
    const size_t top = (size_t)(ny + 1) * P + t, row = (size_t)jb * P + t;
    cur[t] = cur[(size_t)P + t];
    cur[top] = t > si ? cur[top - P] : t == si ? prev[top - P] : own[top - P];
    if (t == si) {
      cur[top - P] = 0.0 + cur[top - P + 1];                     // face column, row ny
      cur[row] = ((0.0 + cur[row + 1]) + cur[row - P]) * 0.5;    // the corner
    }
    if (t > 1 && t < si) cur[row] = 0.0 + cur[row - P];          // face row
  }
}

__global__ __launch_bounds__(256) void mgs_copy_back_kernel(int nx, int ny, int P, int si, int jm, double* __restrict__ dst,
                                                            const double* __restrict__ src) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i > nx + 1 || j > ny + 1) return;
  if ((i == 0 || i == nx + 1) && (j == 0 || j == ny + 1)) return;  // corners: p's own
  const bool solid = i >= 1 && i <= si && j > jm && j <= ny;
  const bool face = j == jm + 1 || i == si;
  if (solid && !face) return;  // interior solid cells: p's own
  const size_t o = (size_t)j * P + i;
  dst[o] = src[o];
}

}  // namespace

template <class Level>
void mg_smooth_launch(const Level* dlv, const Level& L, int l, double* p, const double* f, int colour, void* stream) {
  const dim3 grid(L.nx / 128 + 1, (L.ny + 3) / 4);
  mg_smooth_kernel<typename MgSchemeOf<Level>::type><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(dlv, l, p, f, colour);
}

template <class Level>
void mg_smooth_tile_launch(const Level* dlv, const Level& L, int l, const double* pin, double* pout, const double* f,
                           int nsw, void* stream) {
  const int H = 2 * nsw;
  const dim3 grid(L.nx / (MG_TC - 2 * H) + 1, L.ny / (MG_TR - 2 * H) + 1);
  mg_smooth_tile_kernel<typename MgSchemeOf<Level>::type>
      <<<grid, MG_TILE_THREADS, 0, static_cast<hipStream_t>(stream)>>>(dlv, l, pin, pout, f, nsw);
}

template <class Level>
void mg_restrict_launch(const Level* dlv, const Level& Lc, int l, const double* p, const double* f, double* fc,
                        double* ec, void* stream) {
  const dim3 grid((Lc.nx + 63) / 64, (Lc.ny + 3) / 4);
  mg_restrict_kernel<typename MgSchemeOf<Level>::type><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(dlv, l, p, f, fc, ec);
}

template <class Level>
void mg_prolong_launch(const Level* dlv, const Level& L, int l, double* p, const double* ec, void* stream) {
  const dim3 grid(L.nx / 128 + 1, (L.ny + 3) / 4);
  mg_prolong_kernel<typename MgSchemeOf<Level>::type><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(dlv, l, p, ec);
}

template <class Level>
void mg_tail_launch(const Level* dlv, int l0, int last, int nu1, int nu2, const double* fg, double* eg, void* stream) {
  mg_tail_kernel<typename MgSchemeOf<Level>::type>
      <<<1, MG_TAIL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(dlv, l0, last, nu1, nu2, fg, eg);
}

#define MG_INSTANTIATE(Level)                                                                                              \
  template void mg_smooth_launch<Level>(const Level*, const Level&, int, double*, const double*, int, void*);              \
  template void mg_smooth_tile_launch<Level>(const Level*, const Level&, int, const double*, double*, const double*, int,  \
                                             void*);                                                                       \
  template void mg_restrict_launch<Level>(const Level*, const Level&, int, const double*, const double*, double*, double*, \
                                          void*);                                                                          \
  template void mg_prolong_launch<Level>(const Level*, const Level&, int, double*, const double*, void*);                  \
  template void mg_tail_launch<Level>(const Level*, int, int, int, int, const double*, double*, void*);
MG_INSTANTIATE(MgLevel)
MG_INSTANTIATE(MgoLevel)
MG_INSTANTIATE(MgsLevel)
MG_INSTANTIATE(MgaLevel)
MG_INSTANTIATE(MgoaLevel)
#undef MG_INSTANTIATE

void mgs_refresh_launch(const MgsLevel& L, double* cur, const double* prev, const double* own, void* stream) {
  const int n = std::max(L.nx, L.ny) + 1;
  mgs_refresh_kernel<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(L.nx, L.ny, L.pitch, L.si, L.jm, cur,
                                                                                    prev, own);
}

void mgs_copy_back_launch(const MgsLevel& L, double* dst, const double* src, void* stream) {
  const dim3 grid((L.nx + 2 + 63) / 64, (L.ny + 2 + 3) / 4);
  mgs_copy_back_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(L.nx, L.ny, L.pitch, L.si, L.jm, dst, src);
}


}  // namespace cfd
