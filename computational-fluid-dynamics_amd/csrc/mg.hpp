// mg.hpp — geometric multigrid for the pressure equation: the
// plans (host only, params.cpp) and the launches of mg.hip. No HIP types here,
// so host-only code may include it (streams travel as void*, like comm.hip's).
//
// One set of kernels and one cycle serve five schemes, each an operator with
// its level type and its plan:
//   the cavity and Rayleigh-Benard (CFD_POISSON_MULTIGRID, MgLevel),
//   the channel (CFD_POISSON_MULTIGRID_OPEN, MgoLevel),
//   the backwards-facing step (CFD_POISSON_MULTIGRID_STEP, MgsLevel),
//   the cavity and Rayleigh-Benard at any grid size (CFD_POISSON_MULTIGRID_ANY, MgaLevel),
//   the channel at any grid size (CFD_POISSON_MULTIGRID_OPEN_ANY, MgoaLevel).
// A V(nu1, nu2) cycle: red-black Gauss-Seidel sweeps, residual + restriction
// (the residual never reaches memory), the coarsest level by a fixed number of
// SOR sweeps in one workgroup, the prolongation added to p. Every constant is
// formed on the host; the kernels add, subtract and multiply in the order the
// scheme's numpy restatement under tests/ states, so cycle counts, residuals
// and p are that restatement's, bit for bit.
#pragma once

#include <string>

#include "../../include/cfd_amd.h"

namespace cfd {

constexpr int MG_MAX_LEVELS = 16;
constexpr int MG_COARSE_CELLS = 4096;   // the coarsest level holds at most this many cells
constexpr int MG_LDS_DOUBLES = 18432;   // 144 KiB: p and f of every level of the one-launch tail
constexpr int MG_TAIL_THREADS = 1024;

// What every scheme's level holds.
struct MgLevelBase {
  int nx, ny;        // interior cells
  int pitch;         // global memory: cell (j, i) at j * pitch + i, rows 0 .. ny+1 (128-B aligned rows)
  int lds_p, lds_f;  // one-launch tail: offsets (doubles) of p and f in LDS, rows of nx + 2 (-1: not in the tail)
  int coarse_sweeps; // 4 max(nx, ny): SOR sweeps when this level is the coarsest
  double g;          // ghost factor 1 - 1 / d of the prolongation, towards the Dirichlet side
  double rdiag[16];  // 1 / (the diagonal), indexed by the scheme's mask of a cell's neighbours
  double one_m_omega;  // coarsest SOR: 1 - omega_c, omega_c = 2 / (1 + sin(pi / (max(nx, ny) + 1)))
  double omr[16];      // omega_c * rdiag
};

// The cavity's operator is the reference's (cavity-01.cpp:643-677): Neumann
// west, east and north, and a Dirichlet zero in the bottom ghost row (eps_s =
// j_min = 1 and the ghost row of the fresh pressure field stays 0), i.e. p = 0
// at y = -h/2. Level l (spacing 2^l h) keeps that zero where the finest grid
// has it: its row 1 sees it d_l = 0.5 + 0.5^(l+1) spacings away, so the south
// coefficient of row 1 is cS_l = 1/d_l. A coarse level that moved the zero to
// its own ghost centre (-H/2) makes the cycle diverge. rdiag = 1 / (ew + ee +
// en + cs), index ew | ee << 1 | en << 2 | (row 1) << 3; g is the south ghost's.
// tests/mg_reference.py states every operation.
struct MgLevel : MgLevelBase {
  double h2, ih2;    // 4^l (dx dx) and its reciprocal
  double cS;         // south coefficient of row 1 (1 / d_l)
};

// The channel (DESIGN.md §8 "The channel"): dx != dy, Neumann west / south /
// north and a Dirichlet zero in the east ghost column (channel-01.cpp:642-688).
// Level l has spacings 2^a dx and 2^b dy, cx = 1 / hx^2, cy = 1 / hy^2; column
// nx sees the zero d = 0.5 + 0.5^(a+1) spacings away: east coefficient cE =
// cx / d with neighbour value 0. Levels are semi-coarsened: with r = (hy /
// hx)^2, r > 2 halves x only, r < 1/2 y only, otherwise both. Absent
// neighbours are skipped by selects, so no ghost cell's value reaches a result.
// rdiag = 1 / ((cw + ce) + (cs + cn)), index w | e << 1 | s << 2 | n << 3 (a
// set bit: that neighbour exists); g is the east ghost's.
// tests/mg_open_reference.py states every operation.
enum { MGO_FULL = 0, MGO_X = 1, MGO_Y = 2 };

// (A base of its own, ahead of the shared one: with the coefficients in the head of a level, as before the
// three level types shared a base, the tail kernel keeps its register count - profiles/mg/refactor_resources.txt.)
struct MgoCoef {
  double cx, cy;     // 1 / hx^2, 1 / hy^2
  double cE;         // east coefficient of column nx (cx / d)
};

struct MgoLevel : MgoCoef, MgLevelBase {
  int kind;          // how this level is coarsened to the next: MGO_FULL / MGO_X / MGO_Y (-1: the coarsest)
  int a, b;          // halvings of x and y down to this level
};

// The step: the channel's operator and semi-coarsening on the
// backwards-facing step's fluid cells (backwards_step-01.cpp:872-939 on the
// ghosts and solids 685-740 refresh). Level l has si = step_i >> a, jm =
// inlet_jmax >> b; cell (J, I) is fluid iff I > si or J <= jm, and a neighbour
// exists only inside the grid and fluid. Solid cells are no unknowns: never
// written, never read into a result. The reference's corner solid (jm+1, si) =
// (p_A + p_B) / 2 couples its east fluid cell A = (jm+1, si+1) and its south
// fluid cell B = (jm, si): eliminated, A's west term is (cx/2)(p_B - p_A) and
// B's north term (cy/2)(p_A - p_B), on every level. A and B have one colour;
// both updates of a phase use the pre-phase values: A's thread forms both and
// writes both, B's own skips. tests/mg_step_reference.py states every operation.
struct MgsLevel : MgoLevel {
  int si, jm;        // the block: solid iff i <= si and j > jm
  double chx, chy;   // cx / 2, cy / 2: A's west and B's north coefficient
  double rdA, rdB;   // rdiag for A (cw = chx) and B (cn = chy)
  double omrA, omrB; // omega_c * rdA, omega_c * rdB
};

// The cavity at any size: MgLevel's operator with sizes halved
// rounding up, n_{l+1} = ceil(n_l / 2). In units of the finest spacing, cells
// 1 .. n - 1 of level l are W = 2^l wide and cell n is w = n_0 - (n - 1) W
// (1 <= w <= W): the walls stay where level 0 has them. The operator is the
// finite-volume one in units of ih2: every coefficient 1 (row 1's south cS) but
// across the face between cells n - 1 and n, whose centres are (W + w) / 2
// apart. The restriction is minus the volume-weighted mean of the children's
// residuals, the prolongation linear between the two nearest coarse centres and
// constant beyond the last. A direction with w = W, and an even n where a next
// level follows, is regular: its cells use MgLevel's expressions, so a grid
// whose MgLevel plan ends on a smaller side below 8 gives that plan's bits.
// rdiag = 1 / (((ew + ee) + en) + cs), index cx | cy << 2 with a direction's
// class 0 (cell 1), 1 (2 .. n - 2), 2 (n - 1), 3 (n); every level has n >= 4.
// tests/mg_any_reference.py states every operation.
struct MgaDir {
  int lim;           // cells 2 .. lim - 1 have unit coefficients on both sides: n (w = W) or n - 1
  int last;          // the next level's cell that takes r0 / r1 (its last one), 0: its cells are all regular
  int single;        // that cell has one child (n odd)
  int first;         // cells first .. n take the prolongation weights below (n + 1: none)
  double c_lo;       // east / north coefficient of cell n - 1: 2 W / (W + w)
  double c_hi;       // west / south coefficient of cell n: c_lo W / w
  double r0, r1;     // restriction weights of the last coarse cell's two children: W / (W + w), w / (W + w)
  double pa[3];      // weight of a fine cell's own coarse cell, cells first, first + 1, first + 2
  double pb[3];      // ... of the coarse neighbour on the child's side (0: that term is dropped)
};

struct MgaLevel : MgLevel {
  MgaDir x, y;
};

// The channel at any size: MgoLevel's operator and
// semi-coarsening with sizes halved rounding up, a direction can be halved
// while it has at least 8 cells. Each direction is an MgaDir of its own halving
// count (a for x, b for y): W = 2^a, w = n_0 - (n - 1) W. Here c_lo and c_hi are
// absolute, cx 2 W / (W + w) and that times W / w (cy in y), and a direction the
// level's transfer does not halve has no transfer constants (last 0, first
// n + 1) and is carried over unchanged. Column nx sees the east zero (w + 1) / 2
// finest spacings away: d = (w + 1) / (2 W), cE = (cx / d) (W / w), g = 1 - 1 / d
// - MgoLevel's d, cE and g where w = W. Beyond the last coarse x centre the
// prolongation is linear towards that zero: x.pa[2] = (w + 1) / (w_c + 1) with
// x.pb[2] = 0, where y (a Neumann end) has 1 and 0. rdiag = 1 / ((cw + ce) + (cs +
// cn)), index cx | cy << 2 with MgaLevel's classes; every level has n >= 4 in
// both directions. A cell whose stencil and transfer touch no irregular face
// takes MgoLevel's expressions, so a grid whose MgoLevel plan stops on a size
// below 8 gives that plan's bits. tests/mg_open_any_reference.py states every
// operation.
struct MgoaLevel : MgoLevel {
  MgaDir x, y;
};

template <class Level>
struct MgPlanOf {
  int levels = 0;
  int tail = 0;  // levels tail .. levels-1 run as one launch (tail >= 1)
  Level lv[MG_MAX_LEVELS];
};
using MgPlan = MgPlanOf<MgLevel>;
using MgoPlan = MgPlanOf<MgoLevel>;
using MgsPlan = MgPlanOf<MgsLevel>;
using MgaPlan = MgPlanOf<MgaLevel>;
using MgoaPlan = MgPlanOf<MgoaLevel>;

// The plan of a parameter block, or false with the rule that refused it in
// `why` (host only: params.cpp).
bool mg_make_plan(const cfd_params& p, MgPlan& plan, std::string& why);
bool mgo_make_plan(const cfd_params& p, MgoPlan& plan, std::string& why);
bool mgs_make_plan(const cfd_params& p, MgsPlan& plan, std::string& why);
bool mga_make_plan(const cfd_params& p, MgaPlan& plan, std::string& why);
bool mgoa_make_plan(const cfd_params& p, MgoaPlan& plan, std::string& why);

// Launches (mg.hip), instantiated for the five level types. dlv: the plan's
// levels in device memory; L: the host copy of the level that sizes the grid.
// One colour of a red-black Gauss-Seidel sweep of level l, in place.
template <class Level>
void mg_smooth_launch(const Level* dlv, const Level& L, int l, double* p, const double* f, int colour, void* stream);
// nsw (1..3) whole sweeps of level l in one launch on LDS tiles, pin -> pout (both with zero ghost cells).
template <class Level>
void mg_smooth_tile_launch(const Level* dlv, const Level& L, int l, const double* pin, double* pout, const double* f,
                           int nsw, void* stream);
// f_{l+1} = minus the mean of the residual over each coarse cell's children (four, or two along the one
// direction level l halves); e_{l+1} = 0.
template <class Level>
void mg_restrict_launch(const Level* dlv, const Level& Lc, int l, const double* p, const double* f, double* fc,
                        double* ec, void* stream);
// p_l += the interpolant of e_{l+1} (its ghost layer formed on the fly).
template <class Level>
void mg_prolong_launch(const Level* dlv, const Level& L, int l, double* p, const double* ec, void* stream);
// The sub-cycle over levels l0 .. last in one workgroup, p and f of every level in LDS:
// f_{l0} read from fg, the correction e_{l0} written to eg.
template <class Level>
void mg_tail_launch(const Level* dlv, int l0, int last, int nu1, int nu2, const double* fg, double* eg, void* stream);

// The step only. The reference's refresh (backwards_step-01.cpp:685-740) of level 0's field `cur` (row 0
// of a buffer with L's pitch): the four ghost sides, the block's face row (0 + south), corner (((0 + east) +
// south) / 2) and face column (0 + east). Ghosts that copy a solid cell take an interior solid from
// `own` (the solver's p: the only buffer that holds them) and a face cell's value of before this
// refresh from `prev` (the buffer the previous refresh worked on).
void mgs_refresh_launch(const MgsLevel& L, double* cur, const double* prev, const double* own, void* stream);
// dst <- src over rows 0 .. ny+1 but for the four corner ghosts and the interior solid cells.
void mgs_copy_back_launch(const MgsLevel& L, double* dst, const double* src, void* stream);

}  // namespace cfd
