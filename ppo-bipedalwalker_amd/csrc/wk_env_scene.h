// wk_env_scene.h -- scene props: Square / Triangle / Hexagon rigid bodies (with SmoothCorners)
// added to every walker's body list after the floor (k_env_scene).  On top of wk_env_lane.h: it
// reuses the walker state, joints, integrate, the traced walker pairs and the frame loop of the
// one-lane mapping.  Four translation units instantiate it (given actions / policy, flat / rough
// floor: wk_env_scene_*.hip), one each because a k_env_scene is ~280k instructions and they
// dominate the build's wall time.
//
// Reference: Objects/RigidBodies/{Square,Triangle,Hexagon}.cs (FromSize), Skeleton.cs:33-53
// (SmoothCorners: the vertex list is replaced, the centroid kept), RigidBody.cs:54-113,
// 143-183 (Step, ResolveCollisions, MoveObjects, SetLinear/AngularVelocity,
// AddAcceleration), Environment.cs:126-143 (StepObjects over List<RigidBody>).
//
// A prop has up to 24 vertices and its vertex count is the same for every walker, so the
// runtime vertex loops are wave-uniform.  Its state lives in LDS for the whole launch as
// per-lane columns ([field][64 lanes]: lane l's field f at lds[64 f + l], conflict-free),
// loaded from / stored to HBM once per launch.  The walker's own bodies stay in registers
// (Poly<N>); the pair routines below are written once over both kinds through overloads:
// compile-time-unrolled for a register polygon, a runtime loop for an LDS polygon.
// Arithmetic is op-for-op the reference's (same association as resolve_pair / the oracle),
// so walkers with props stay bit-exact with the CPU restatement.

#pragma once
#include "wk_env_lane.h"

namespace wk {

// an LDS-resident prop polygon: x(i) at b[64 i], y(i) at b[64 (n + i)], then cx, cy, vx,
// vy, w, angle (SceneDev::off gives the first field of each prop)
struct LPoly {
  float* b;
  int n;
  float* box;  // cached bounding box min x, min y, max x, max y at box[0], [64], [128], [192]
  DEV float x(int i) const { return b[64 * i]; }
  DEV float y(int i) const { return b[64 * (n + i)]; }
  DEV float& xr(int i) const { return b[64 * i]; }
  DEV float& yr(int i) const { return b[64 * (n + i)]; }
  DEV float& f(int k) const { return b[64 * (2 * n + k)]; }  // 0 cx, 1 cy, 2 vx, 3 vy, 4 w, 5 th
};
DEV float pcx(const LPoly& p) { return p.f(0); }
DEV float pcy(const LPoly& p) { return p.f(1); }
template <int N> DEV float pcx(const Poly<N>& p) { return p.cx; }
template <int N> DEV float pcy(const Poly<N>& p) { return p.cy; }

DEV Dyn load_pdyn(const LPoly& p) { Dyn d; d.vx = p.f(2); d.vy = p.f(3); d.w = p.f(4); d.th = p.f(5); return d; }
DEV void store_pdyn(const LPoly& p, const Dyn& d) { p.f(2) = d.vx; p.f(3) = d.vy; p.f(4) = d.w; p.f(5) = d.th; }

// ---- per-kind primitives ----
template <int N, class F> DEV void for_edges(const Poly<N>& P, F fn) {
#pragma unroll
  for (int i = 0; i < N; i++) fn(P.x[i], P.y[i], P.x[(i + 1) % N], P.y[(i + 1) % N]);
}
template <class F> DEV void for_edges(const LPoly& P, F fn) {
#pragma unroll 1
  for (int i = 0; i < P.n; i++) {
    const int i1 = i + 1 == P.n ? 0 : i + 1;
    fn(P.x(i), P.y(i), P.x(i1), P.y(i1));
  }
}
// SATCollision.Project (:63-76) by value (see project2)
template <int N> DEV void project_g(const Poly<N>& P, float ax, float ay, float& mn, float& mx) {
  mn = FLT_MAX; mx = -FLT_MAX;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const float p = ax * P.x[i] + ay * P.y[i];
    mn = __builtin_fminf(mn, p);
    mx = __builtin_fmaxf(mx, p);
  }
}
DEV void project_g(const LPoly& P, float ax, float ay, float& mn, float& mx) {
  mn = FLT_MAX; mx = -FLT_MAX;
#pragma unroll 2
  for (int i = 0; i < P.n; i++) {
    const float p = ax * P.x(i) + ay * P.y(i);
    mn = __builtin_fminf(mn, p);
    mx = __builtin_fmaxf(mx, p);
  }
}
template <int N> DEV void aabb_g(const Poly<N>& P, float& mnx, float& mny, float& mxx, float& mxy) {
  aabb(P, mnx, mny, mxx, mxy);
}
// BoundingBox.Update (Skeleton.cs:127-130) runs after every Move and Rotate: the box is
// cached in LDS and refreshed exactly then (a move translates it: round-to-nearest addition
// is monotonic, so min_i fl(x_i + d) = fl(min_i x_i + d))
DEV void aabb_g(const LPoly& P, float& mnx, float& mny, float& mxx, float& mxy) {
  mnx = P.box[0]; mny = P.box[64]; mxx = P.box[128]; mxy = P.box[192];
}
DEV void box_refresh(const LPoly& P) {
  float maxX = -FLT_MAX, maxY = -FLT_MAX, minX = FLT_MAX, minY = FLT_MAX;
#pragma unroll 2
  for (int i = 0; i < P.n; i++) {
    const float x = P.x(i), y = P.y(i);
    maxX = __builtin_fmaxf(maxX, x); maxY = __builtin_fmaxf(maxY, y);
    minX = __builtin_fminf(minX, x); minY = __builtin_fminf(minY, y);
  }
  P.box[0] = minX; P.box[64] = minY; P.box[128] = maxX; P.box[192] = maxY;
}
template <int N> DEV void move_g(Poly<N>& P, V2 d) { move(P, d); }
DEV void move_g(const LPoly& P, V2 d) {  // Skeleton.Move (:76-85)
#pragma unroll 2
  for (int i = 0; i < P.n; i++) { P.xr(i) = P.x(i) + d.x; P.yr(i) = P.y(i) + d.y; }
  P.f(0) = P.f(0) + d.x;
  P.f(1) = P.f(1) + d.y;
  P.box[0] = P.box[0] + d.x; P.box[64] = P.box[64] + d.y;
  P.box[128] = P.box[128] + d.x; P.box[192] = P.box[192] + d.y;
}
// GetSignificantFace / GetSignificantVertex (ContactPoints.cs:79-113) on an LDS polygon:
// first strict minimum of the projections; index -1 (no projection below MaxValue) keeps
// Vector2.Zero and the neighbours 0 and Mod(-2, n) = n - 2.  Normalize may see a zero edge
// (a degenerate prop): the guarded vnormalize returns its NaN, as Vector2.Normalize does.
template <int N> DEV void sig_face_g(const Poly<N>& P, V2 n, V2& fa, V2& fb, V2& fmax) {
  significant_face<N, true>(P, n, fa, fb, fmax);
}
DEV void sig_face_g(const LPoly& P, V2 n, V2& fa, V2& fb, V2& fmax) {
  float mind = FLT_MAX;
  int idx = -1;
#pragma unroll 2
  for (int i = 0; i < P.n; i++) {
    const float p = P.x(i) * n.x + P.y(i) * n.y;
    if (p < mind) { mind = p; idx = i; }
  }
  const V2 sig = idx >= 0 ? mk(P.x(idx), P.y(idx)) : mk(0.0f, 0.0f);
  const int ia = idx + 1 == P.n ? 0 : idx + 1;
  const int ib = idx >= 1 ? idx - 1 : idx + P.n - 1;
  const V2 va = mk(P.x(ia), P.y(ia)), vb = mk(P.x(ib), P.y(ib));
  const V2 after = vnormalize(vsub(sig, va));
  const V2 before = vnormalize(vsub(sig, vb));
  const bool first = vdot(n, before) >= vdot(n, after);
  fa = first ? sig : va;
  fb = first ? vb : sig;
  fmax = sig;
}

// ---- register copy of an LDS prop of at most RPV vertices ----
// Inside one RigidBody.Step a prop takes part in up to (walker parts + floor + props) pairs,
// each projecting it once per SAT axis: read through LDS that is ~n^2 dependent LDS round trips
// per pair at one wave per SIMD.  Every prop of up to 8 vertices (the base shapes and the
// once-smoothed square and triangle) is therefore read into registers once, and every change
// is written through to LDS (the source of truth) with the same IEEE ops, so the results are
// bit-identical to the LPoly path.  Vertex loops are unrolled to RPV with a wave-uniform exit
// (the vertex count is the same for every walker).  Reads past n stay inside the prop's own
// 2 n + 6 fields (n >= 2) or the box rows that follow them.
constexpr int RPV = 8;
struct RPoly {
  float x[RPV], y[RPV], cx, cy;
  float bx0, by0, bx1, by1;  // the cached bounding box (as LPoly::box)
  int n;
  LPoly L;
};
DEV RPoly rpoly_load(const LPoly& L) {
  RPoly R;
  R.n = L.n;
  R.L = L;
#pragma unroll
  for (int i = 0; i < RPV; i++) { R.x[i] = L.b[64 * i]; R.y[i] = L.b[64 * (L.n + i)]; }
  R.cx = L.f(0);
  R.cy = L.f(1);
  R.bx0 = L.box[0]; R.by0 = L.box[64]; R.bx1 = L.box[128]; R.by1 = L.box[192];
  return R;
}
DEV float pcx(const RPoly& p) { return p.cx; }
DEV float pcy(const RPoly& p) { return p.cy; }
// v[j] for a runtime j < RPV: bit-mask ORs over the unrolled registers (a compare/select
// chain gets folded by LLVM into a load through a selected address, which moves the register
// copies -- and the walker state with them -- to scratch memory; cf. pick)
DEV V2 rp_vertex(const RPoly& P, int j) {
  uint32_t bx = 0u, by = 0u;
#pragma unroll
  for (int i = 0; i < RPV; i++) {
    const uint32_t m = j == i ? 0xffffffffu : 0u;
    bx |= m & __float_as_uint(P.x[i]);
    by |= m & __float_as_uint(P.y[i]);
  }
  return mk(__uint_as_float(bx), __uint_as_float(by));
}
template <class F> DEV void for_edges(const RPoly& P, F fn) {
#pragma unroll
  for (int i = 0; i < RPV; i++) {
    if (i < P.n) {
      const bool wrap = i + 1 == P.n || i + 1 == RPV;
      fn(P.x[i], P.y[i], wrap ? P.x[0] : P.x[(i + 1) % RPV], wrap ? P.y[0] : P.y[(i + 1) % RPV]);
    }
  }
}
DEV void project_g(const RPoly& P, float ax, float ay, float& mn, float& mx) {
  mn = FLT_MAX; mx = -FLT_MAX;
#pragma unroll
  for (int i = 0; i < RPV; i++) {
    if (i < P.n) {
      const float p = ax * P.x[i] + ay * P.y[i];
      mn = __builtin_fminf(mn, p);
      mx = __builtin_fmaxf(mx, p);
    }
  }
}
DEV void aabb_g(const RPoly& P, float& mnx, float& mny, float& mxx, float& mxy) {
  mnx = P.bx0; mny = P.by0; mxx = P.bx1; mxy = P.by1;
}
DEV void move_g(RPoly& P, V2 d) {  // Skeleton.Move, written through to the LDS prop
#pragma unroll
  for (int i = 0; i < RPV; i++) {
    P.x[i] = P.x[i] + d.x;  // (past n: harmless arithmetic on copies, never stored)
    P.y[i] = P.y[i] + d.y;
    if (i < P.n) {
      P.L.xr(i) = P.x[i];
      P.L.yr(i) = P.y[i];
    }
  }
  P.cx = P.cx + d.x;
  P.cy = P.cy + d.y;
  P.L.f(0) = P.cx;
  P.L.f(1) = P.cy;
  P.bx0 = P.bx0 + d.x; P.by0 = P.by0 + d.y; P.bx1 = P.bx1 + d.x; P.by1 = P.by1 + d.y;
  P.L.box[0] = P.bx0; P.L.box[64] = P.by0; P.L.box[128] = P.bx1; P.L.box[192] = P.by1;
}
// GetSignificantFace on the register copy: the same first strict minimum, neighbours and
// index -1 fallback (Zero vertex, neighbours 0 and n - 2) as the LPoly version
DEV void sig_face_g(const RPoly& P, V2 n, V2& fa, V2& fb, V2& fmax) {
  float mind = FLT_MAX;
  const V2 vb0 = rp_vertex(P, P.n - 2), vlast = rp_vertex(P, P.n - 1);
  uint32_t sx = 0u, sy = 0u;  // Zero
  uint32_t ax = __float_as_uint(P.x[0]), ay = __float_as_uint(P.y[0]);
  uint32_t bx = __float_as_uint(vb0.x), by = __float_as_uint(vb0.y);
#pragma unroll
  for (int i = 0; i < RPV; i++) {
    const float p = P.x[i] * n.x + P.y[i] * n.y;
    const bool lt = i < P.n && p < mind;
    const uint32_t m = lt ? 0xffffffffu : 0u;
    mind = lt ? p : mind;
    const bool wrap = i + 1 == P.n || i + 1 == RPV;
    const float nx = wrap ? P.x[0] : P.x[(i + 1) % RPV], ny = wrap ? P.y[0] : P.y[(i + 1) % RPV];
    const float px = i == 0 ? vlast.x : P.x[(i + RPV - 1) % RPV];
    const float py = i == 0 ? vlast.y : P.y[(i + RPV - 1) % RPV];
    sx = bsel(m, P.x[i], sx); sy = bsel(m, P.y[i], sy);
    ax = bsel(m, nx, ax);     ay = bsel(m, ny, ay);
    bx = bsel(m, px, bx);     by = bsel(m, py, by);
  }
  const V2 sig = mk(__uint_as_float(sx), __uint_as_float(sy));
  const V2 va = mk(__uint_as_float(ax), __uint_as_float(ay)), vb = mk(__uint_as_float(bx), __uint_as_float(by));
  const V2 after = vnormalize(vsub(sig, va));
  const V2 before = vnormalize(vsub(sig, vb));
  const bool first = vdot(n, before) >= vdot(n, after);
  fa = first ? sig : va;
  fb = first ? vb : sig;
  fmax = sig;
}

// ---- SAT (SATCollision.cs:15-104) over either kind ----
// AxisChecks(P's edges, Q), branch-free as axis_pass: a zero axis is skipped, the first
// strict minimum depth wins; the axis is normalised with the guarded Normalize (identical
// bits to vnormalize_edge on every edge a rigid walker polygon can have).
template <class PP, class PQ>
DEV void axis_pass_g(const PP& P, const PQ& Q, bool& sep, V2& normal, float& depth) {
  for_edges(P, [&](float x0, float y0, float x1, float y1) {
    const float ex = x1 - x0, ey = y1 - y0;
    V2 axis = mk(-ey, ex);
    const bool valid = !(axis.x == 0.0f && axis.y == 0.0f);
    axis = vnormalize(axis);
    float pmin, pmax, qmin, qmax;
    project_g(P, axis.x, axis.y, pmin, pmax);
    project_g(Q, axis.x, axis.y, qmin, qmax);
    const float temp = __builtin_fminf(qmax - pmin, pmax - qmin);
    const bool overlapping = (pmin < qmax) && (qmin < pmax);
    sep = sep || (valid && !overlapping);
    const bool take = valid && overlapping && temp < depth;
    depth = take ? temp : depth;
    normal.x = take ? axis.x : normal.x;
    normal.y = take ? axis.y : normal.y;
  });
}
// The flat floor box (Environment.cs:211-226) as the other body of a prop's pair: the same
// values as the generic path on its Poly<4>, from closed forms (cf. sat_floor).  Its vertices
// are all combinations of x in {-50, 1050} and y in {900, 1050}, so its projection on any
// axis is fl(min fl(ax x) + min fl(ay y)) .. fl(max + max) (round-to-nearest addition is
// monotonic); its edges normalise to exactly (1,+0), (-0,1), (-1,+0), (-0,-1), onto which
// the prop projects to its cached bounding box's extents (equal in value; the sign of a zero
// never reaches a depth).  It is static: it never moves.
struct FlatFloor { Poly<4> p; };
DEV float pcx(const FlatFloor& f) { return f.p.cx; }
DEV float pcy(const FlatFloor& f) { return f.p.cy; }
DEV void project_g(const FlatFloor&, float ax, float ay, float& mn, float& mx) {
  const float x0 = ax * -50.0f, x1 = ax * 1050.0f, y0 = ay * 900.0f, y1 = ay * 1050.0f;
  mn = __builtin_fminf(x0, x1) + __builtin_fminf(y0, y1);
  mx = __builtin_fmaxf(x0, x1) + __builtin_fmaxf(y0, y1);
}
DEV void aabb_g(const FlatFloor& f, float& mnx, float& mny, float& mxx, float& mxy) { aabb(f.p, mnx, mny, mxx, mxy); }
DEV void move_g(FlatFloor&, V2) {}
DEV void sig_face_g(const FlatFloor& f, V2 n, V2& fa, V2& fb, V2& fmax) { significant_face<4, true>(f.p, n, fa, fb, fmax); }
// AxisChecks(floor, Q): the floor's four edges in vertex order
template <class PQ>
DEV void axis_pass_g(const FlatFloor&, const PQ& Q, bool& sep, V2& normal, float& depth) {
  float mnx, mny, mxx, mxy;
  aabb_g(Q, mnx, mny, mxx, mxy);
  auto ax = [&](float pmin, float pmax, float qmin, float qmax, float nx, float ny) {
    const float temp = __builtin_fminf(qmax - pmin, pmax - qmin);
    const bool overlapping = (pmin < qmax) && (qmin < pmax);
    sep = sep || !overlapping;
    const bool take = overlapping && temp < depth;
    depth = take ? temp : depth;
    normal.x = take ? nx : normal.x;
    normal.y = take ? ny : normal.y;
  };
  ax(-50.0f, 1050.0f, mnx, mxx, 1.0f, 0.0f);
  ax(900.0f, 1050.0f, mny, mxy, -0.0f, 1.0f);
  ax(-1050.0f, 50.0f, -mxx, -mnx, -1.0f, 0.0f);
  ax(-1050.0f, -900.0f, -mxy, -mny, -0.0f, -1.0f);
}

template <class PA, class PB>
DEV bool sat_g(const PA& A, const PB& B, V2& normal, float& depth) {
  normal = mk(0.0f, 0.0f);
  depth = FLT_MAX;
  bool sep = false;
  axis_pass_g(A, B, sep, normal, depth);
  axis_pass_g(B, A, sep, normal, depth);
  V2 dir = mk(pcx(B) - pcx(A), pcy(B) - pcy(A));
  if (vdot(dir, normal) > 0.0f) normal = vmul(normal, -1.0f);
  return !sep;
}

// GetContactPoints (ContactPoints.cs:13-53) over either kind (cf. contact_points)
template <class PA, class PB>
DEV int contact_points_g(const PA& A, const PB& B, V2 normal, V2& c0, V2& c1) {
  V2 ra, rb, rmax, ia, ib, imax;
  sig_face_g(A, normal, ra, rb, rmax);
  V2 rf = vsub(rb, ra);
  sig_face_g(B, vneg(normal), ia, ib, imax);
  V2 iv = vsub(ib, ia);
  if (fabsf(vdot(rf, normal)) > fabsf(vdot(iv, normal))) {
    V2 t;
    t = ra; ra = ia; ia = t;
    t = rb; rb = ib; ib = t;
    t = rmax; rmax = imax; imax = t;
    rf = vsub(rb, ra);
  }
  rf = vnormalize(rf);
  float offset = vdot(rf, ra);
  V2 p0 = mk(0.0f, 0.0f), p1 = mk(0.0f, 0.0f);
  const int k1 = clip_vectors(ia, ib, rf, offset, p0, p1);
  offset = vdot(rf, rb);
  V2 q0 = mk(0.0f, 0.0f), q1 = mk(0.0f, 0.0f);
  const int k2 = clip_vectors(p0, p1, vneg(rf), -offset, q0, q1);
  if (k1 < 2 || k2 < 2) return 0;
  V2 refn = mk(rf.y, -rf.x);
  float maximum = vdot(refn, rmax);
  int cnt = 2;
  if (vdot(refn, q0) - maximum < 0.0f) { q0 = q1; cnt = 1; }
  V2 last = cnt == 2 ? q1 : q0;
  if (vdot(refn, last) - maximum < 0.0f) cnt = cnt == 2 ? 1 : 0;
  c0 = q0;
  c1 = q1;
  return cnt;
}

// RigidBody.ResolveCollisions body for (this = A, other = B) with either kind (cf.
// resolve_pair): B static -> A takes the whole correction (MoveObjects :99-113); B a floor
// body -> A.Collided (:75).  Impulses go to both bodies (Impulses.ApplyImpulses :57-82): a
// static prop has zero inverse mass and inertia, so its velocities are unchanged.
template <class PA, class PB>
DEV void resolve_g(PA& A, Dyn& dA, const Mat& mA, PB& B, Dyn& dB, const Mat& mB, bool bstatic,
                   bool bfloor, bool& colA) {
  float a0x, a0y, a1x, a1y, b0x, b0y, b1x, b1y;
  aabb_g(A, a0x, a0y, a1x, a1y);
  aabb_g(B, b0x, b0y, b1x, b1y);
  if (!(a0x < b1x && a1x > b0x && a0y < b1y && a1y > b0y)) return;
  if (bfloor) colA = true;
  V2 n;
  float depth;
  if (!sat_g(A, B, n, depth)) return;
  V2 c0, c1;
  const int nc = contact_points_g(A, B, n, c0, c1);
  if (bstatic) {
    move_g(A, vmul(n, depth));
  } else {
    move_g(A, vdiv(vmul(n, depth), 2.0f));
    move_g(B, vdiv(vmul(vneg(n), depth), 2.0f));
  }
  if (nc == 0) return;
  const float e = net_maxf(mA.e, mB.e);
  const float mu = net_minf(mA.mu, mB.mu);
  const V2 contact = nc == 2 ? vdiv(vadd(c0, c1), 2.0f) : c0;
  Body bA{pcx(A), pcy(A), &dA, mA.im, mA.ii};
  Body bB{pcx(B), pcy(B), &dB, mB.im, mB.ii};
  V2 rA, rB, rAF, rBF;
  const float j = calc_impulse(bA, bB, contact, 1.0f + e, n, rA, rB);
  const V2 tangent = mk(-n.y, n.x);
  const float jf = calc_impulse(bA, bB, contact, mu, tangent, rAF, rBF);
  apply_impulses<false>(bA, bB, n, j, rA, rB);
  apply_impulses<false>(bA, bB, tangent, jf, rAF, rBF);
}

DEV LPoly scene_prop(const SceneDev& S, float* col, int k) {
  return LPoly{col + 64 * S.off[k], S.nv[k], col + 64 * (SCENE_FIELDS + 4 * k)};
}
DEV Mat scene_mat(const SceneDev& S, int k) { return Mat{S.im[k], S.ii[k], S.e[k], S.mu[k]}; }
// the same for a per-lane (divergent) prop index: select chains over the kernel arguments
DEV int sel_i(const int (&a)[SCENE_MAX_PROPS], int k) {
  int v = a[0];
#pragma unroll
  for (int i = 1; i < SCENE_MAX_PROPS; i++) v = k == i ? a[i] : v;
  return v;
}
DEV float sel_f(const float (&a)[SCENE_MAX_PROPS], int k) {
  float v = a[0];
#pragma unroll
  for (int i = 1; i < SCENE_MAX_PROPS; i++) v = k == i ? a[i] : v;
  return v;
}
DEV LPoly scene_prop_v(const SceneDev& S, float* col, int k) {
  return LPoly{col + 64 * sel_i(S.off, k), sel_i(S.nv, k), col + 64 * (SCENE_FIELDS + 4 * k)};
}
DEV Mat scene_mat_v(const SceneDev& S, int k) {
  return Mat{sel_f(S.im, k), sel_f(S.ii, k), sel_f(S.e, k), sel_f(S.mu, k)};
}
DEV bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }
// the first prop q >= from (q != skip) whose cached bounding box overlaps (a0, a1), else
// n_props: every prop's box is read at once (the loads of absent props stay inside the
// allocation and are masked), no per-prop LDS round trip
DEV int next_overlap(const float* col, int n_props, int from, int skip, float a0x, float a0y,
                     float a1x, float a1y) {
  uint32_t m = 0u;
#pragma unroll
  for (int q = 0; q < SCENE_MAX_PROPS; q++) {
    const float* bx = col + 64 * (SCENE_FIELDS + 4 * q);
    const bool ov = a0x < bx[64 * 2] && a1x > bx[0] && a0y < bx[64 * 3] && a1y > bx[64];
    m |= (ov && q >= from && q < n_props && q != skip) ? (1u << q) : 0u;
  }
  return m ? __builtin_ctz(m) : n_props;
}

// (part, prop k) with the prop as an exact Poly<N> register copy (written back to LDS after
// the pair when it can move) -- for a round in which every active lane meets the same prop k
// of N vertices (wave-uniform), the common case: every walker carries the same props
template <int N, int NP>
DEV void resolve_part_prop_n(Poly<NP>& P, Dyn& D, const Mat& m, const LPoly& Q, Dyn& dq,
                             const Mat& mq, bool st) {
  Poly<N> B;
#pragma unroll
  for (int i = 0; i < N; i++) { B.x[i] = Q.x(i); B.y[i] = Q.y(i); }
  B.cx = Q.f(0);
  B.cy = Q.f(1);
  bool col_unused = false;
  resolve_g(P, D, m, B, dq, mq, st, false, col_unused);
  if (!st) {
#pragma unroll
    for (int i = 0; i < N; i++) { Q.xr(i) = B.x[i]; Q.yr(i) = B.y[i]; }
    Q.f(0) = B.cx;
    Q.f(1) = B.cy;
    float mnx, mny, mxx, mxy;
    aabb(B, mnx, mny, mxx, mxy);
    Q.box[0] = mnx; Q.box[64] = mny; Q.box[128] = mxx; Q.box[192] = mxy;
  }
}

// a walker part's candidate pairs against every prop, in list order
template <int N>
DEV void part_vs_props(Poly<N>& P, Dyn& D, const Mat& m, const SceneDev& S, float* col) {
  bool col_unused = false;
  // Each lane walks the props in list order on its own: a scan past the props whose bounding
  // box misses (cheap, lane-local), then one collision resolution per round for every lane
  // that found one -- each lane on its own next prop.  The wave runs as many resolutions as
  // its busiest lane needs, not one per prop that any lane touches (ballot-driven exit).
  // Per lane the sequence is the reference's: every bounding-box test sees the state left by
  // the previous pair.
  int k = 0;
#pragma unroll 1
  while (true) {
    float a0x, a0y, a1x, a1y;
    aabb(P, a0x, a0y, a1x, a1y);
    k = next_overlap(col, S.n_props, k, -1, a0x, a0y, a1x, a1y);
    const bool hit = k < S.n_props;
    if (!wave_any(hit)) break;
    if (hit) {
      LPoly Q = scene_prop_v(S, col, k);
      Dyn dq = load_pdyn(Q);
      const Mat mq = scene_mat_v(S, k);
      const bool st = sel_i(S.stat, k) != 0;
      // every active lane at the same prop: its exact vertex count (a scalar branch)
      const int kf = __builtin_amdgcn_readfirstlane(k);
      const bool uni = __builtin_amdgcn_ballot_w64(k == kf) == __builtin_amdgcn_ballot_w64(true);
      const int nf = uni ? sel_i(S.nv, kf) : 0;
      if (nf == 4) resolve_part_prop_n<4>(P, D, m, Q, dq, mq, st);
      else if (nf == 6) resolve_part_prop_n<6>(P, D, m, Q, dq, mq, st);
      else if (nf == 8) resolve_part_prop_n<8>(P, D, m, Q, dq, mq, st);
      else if (Q.n <= RPV) {
        RPoly R = rpoly_load(Q);
        resolve_g(P, D, m, R, dq, mq, st, false, col_unused);
      } else {
        resolve_g(P, D, m, Q, dq, mq, st, false, col_unused);
      }
      store_pdyn(Q, dq);
      k++;
    }
  }
}

// prop k's candidate pairs (RigidBody.ResolveCollisions over the list) with A its register
// copy or its LDS polygon
template <bool ROUGH, class PA>
DEV void prop_pairs(EnvState& s, const Mat& mp, const Mat& mb, const SceneDev& S, float* col,
                    int k, PA& A, Dyn& d, const float* ter) {
  const Mat ma = scene_mat(S, k);
  bool col_unused = false;
  Poly<4> fl;
  floor_poly(fl);
  Dyn dfl;
  zero_dyn(dfl);
  const Mat mf{0.0f, 0.0f, 0.3f, 1.0f};
  // (the walker's five parts stay a fixed sequence: a per-lane walk over them, with the part
  // picked and written back by bit masks, measured slower -- prop-walker contacts are rare)
  auto walker = [&]() __attribute__((always_inline)) {
    resolve_g(A, d, ma, s.lll, s.dlll, mp, false, false, col_unused);
    resolve_g(A, d, ma, s.llu, s.dllu, mp, false, false, col_unused);
    resolve_g(A, d, ma, s.body, s.dbody, mb, false, false, col_unused);
    resolve_g(A, d, ma, s.rll, s.drll, mp, false, false, col_unused);
    resolve_g(A, d, ma, s.rlu, s.drlu, mp, false, false, col_unused);
  };
  if (!s.post) walker();
  if constexpr (ROUGH) {  // CreateRoughFloor's 10 static segments, in list order
#pragma unroll 1
    for (int q = 0; q < 10; q++) {
      Poly<4> seg;
      rough_segment(seg, q, ter[q * 64], ter[(q + 1) * 64]);
      resolve_g(A, d, ma, seg, dfl, mf, true, true, col_unused);
    }
  } else {
    FlatFloor ff{fl};
    resolve_g(A, d, ma, ff, dfl, mf, true, true, col_unused);
  }
  // the other props, each lane walking them on its own (see part_vs_props)
  int j = 0;
#pragma unroll 1
  while (true) {
    float a0x, a0y, a1x, a1y;
    aabb_g(A, a0x, a0y, a1x, a1y);
    j = next_overlap(col, S.n_props, j, k, a0x, a0y, a1x, a1y);
    const bool hit = j < S.n_props;
    if (!wave_any(hit)) break;
    if (hit) {
      LPoly B = scene_prop_v(S, col, j);
      Dyn db = load_pdyn(B);
      const Mat mj = scene_mat_v(S, j);
      const bool st = sel_i(S.stat, j) != 0;
      if (B.n <= RPV) {
        RPoly RB = rpoly_load(B);
        resolve_g(A, d, ma, RB, db, mj, st, false, col_unused);
      } else {
        resolve_g(A, d, ma, B, db, mj, st, false, col_unused);
      }
      store_pdyn(B, db);
      j++;
    }
  }
  if (s.post) walker();
}

// The rest of prop k's RigidBody.Step for a prop of exactly N vertices (wave-uniform): move,
// rotate and every pair on a Poly<N> register copy -- SAT, contact faces and bounding boxes
// unrolled over the exact vertex count instead of RPV masked slots -- written back to LDS
// once at the end.  Nothing in between reads prop k from LDS: its pairs read the *other*
// props, and the overlap scan skips k.  Same operations as the RPoly path (move, then
// Skeleton.Rotate about the moved centroid, boxes from the vertices), so the same bits.
template <int N, bool ROUGH>
DEV void prop_step_n(EnvState& s, const Mat& mp, const Mat& mb, const SceneDev& S, float* col,
                     int k, const LPoly& L, Dyn& d, V2 mv, float angle, const float* ter) {
  Poly<N> A;
#pragma unroll
  for (int i = 0; i < N; i++) { A.x[i] = L.x(i); A.y[i] = L.y(i); }
  A.cx = L.f(0);
  A.cy = L.f(1);
  move(A, mv);
  rotate(A, angle);
  prop_pairs<ROUGH>(s, mp, mb, S, col, k, A, d, ter);
#pragma unroll
  for (int i = 0; i < N; i++) { L.xr(i) = A.x[i]; L.yr(i) = A.y[i]; }
  L.f(0) = A.cx;
  L.f(1) = A.cy;
  float mnx, mny, mxx, mxy;
  aabb(A, mnx, mny, mxx, mxy);
  L.box[0] = mnx; L.box[64] = mny; L.box[128] = mxx; L.box[192] = mxy;
}

// RigidBody.Step of prop k (RigidBody.cs:54-61): StepLinearVelocity; a static prop stops
// there; else StepAngularVelocity and ResolveCollisions against the list: episode 0
// [LLL, LLU, Body, RLL, RLU, Floor, props], after a reset [Floor, props, LLL, ..., RLU]
template <bool ROUGH>
DEV void prop_step(EnvState& s, const Mat& mp, const Mat& mb, float dt, const SceneDev& S,
                   float* col, int k, const float* ter) {
  LPoly A = scene_prop(S, col, k);
  Dyn d = load_pdyn(A);
  d.vx = d.vx + S.adx[k];
  d.vy = d.vy + S.ady[k];
  const V2 mv = mk(d.vx * dt, d.vy * dt);
  if (S.stat[k]) { move_g(A, mv); store_pdyn(A, d); return; }
  d.th = d.th + d.w * dt;
  d.th = wrap_angle(d.th);
  // Skeleton.Rotate about the stored centroid (cf. rotate)
  const float angle = d.w * dt;
  if (A.n == 4 || A.n == 6 || A.n == 8) {  // the base square, hexagon and smoothed triangle / square
    if (A.n == 4) prop_step_n<4, ROUGH>(s, mp, mb, S, col, k, A, d, mv, angle, ter);
    else if (A.n == 6) prop_step_n<6, ROUGH>(s, mp, mb, S, col, k, A, d, mv, angle, ter);
    else prop_step_n<8, ROUGH>(s, mp, mb, S, col, k, A, d, mv, angle, ter);
    store_pdyn(A, d);
    return;
  }
  double sd, cd;
  if (__builtin_fabsf(angle) <= 0.25f) wk_sincos_small((double)angle, &sd, &cd);
  else sincos((double)angle, &sd, &cd);
  const float c = (float)cd, sn = (float)sd;
  const float m11 = c, m12 = sn, m21 = -sn, m22 = c;
  if (A.n <= RPV) {  // move, rotate and bounding box on the register copy, one write-back
    RPoly R = rpoly_load(A);
#pragma unroll
    for (int i = 0; i < RPV; i++) { R.x[i] = R.x[i] + mv.x; R.y[i] = R.y[i] + mv.y; }
    R.cx = R.cx + mv.x;
    R.cy = R.cy + mv.y;
    float maxX = -FLT_MAX, maxY = -FLT_MAX, minX = FLT_MAX, minY = FLT_MAX;
#pragma unroll
    for (int i = 0; i < RPV; i++) {
      const float px = R.x[i] - R.cx, py = R.y[i] - R.cy;
      const float tx = (px * m11) + (py * m21) + 0.0f;
      const float ty = (px * m12) + (py * m22) + 0.0f;
      R.x[i] = tx + R.cx;
      R.y[i] = ty + R.cy;
      if (i < R.n) {
        A.xr(i) = R.x[i];
        A.yr(i) = R.y[i];
        maxX = __builtin_fmaxf(maxX, R.x[i]); maxY = __builtin_fmaxf(maxY, R.y[i]);
        minX = __builtin_fminf(minX, R.x[i]); minY = __builtin_fminf(minY, R.y[i]);
      }
    }
    A.f(0) = R.cx;
    A.f(1) = R.cy;
    A.box[0] = minX; A.box[64] = minY; A.box[128] = maxX; A.box[192] = maxY;
    R.bx0 = minX; R.by0 = minY; R.bx1 = maxX; R.by1 = maxY;
    prop_pairs<ROUGH>(s, mp, mb, S, col, k, R, d, ter);
  } else {
    move_g(A, mv);
    const float cx = A.f(0), cy = A.f(1);
#pragma unroll 2
    for (int i = 0; i < A.n; i++) {
      const float px = A.x(i) - cx, py = A.y(i) - cy;
      const float tx = (px * m11) + (py * m21) + 0.0f;
      const float ty = (px * m12) + (py * m22) + 0.0f;
      A.xr(i) = tx + cx;
      A.yr(i) = ty + cy;
    }
    box_refresh(A);
    prop_pairs<ROUGH>(s, mp, mb, S, col, k, A, d, ter);
  }
  store_pdyn(A, d);
}

// one substep of StepObjects with props (cf. substep<TRACE, 1, false>): the walker's
// traced pairs are unchanged; each part additionally meets every prop right after the
// floor, and the props step after the floor (episode 0: after the walker, post-reset:
// before it)
// ROUGH: the floor bodies are CreateRoughFloor's 10 segments (ter: this walker's terrain
// column in LDS, stride 64) -- list order [walker, segments, props], after a reset
// [segments, props, walker]
template <bool TRACE, bool ROUGH = false>
DEV void substep_scene(EnvState& s, const Mat& mp, const Mat& mb, float dt, float adx, float ady,
                       PairTraceDev* tr, const SceneDev& S, float* col, const float* ter) {
  joint_step<5, 6, 1, 4, TRACE>(s.body, s.dbody, mb, s.llu, s.dllu, mp, tr, 0);
  joint_step<5, 6, 1, 4, TRACE>(s.body, s.dbody, mb, s.rlu, s.drlu, mp, tr, 1);
  joint_step<6, 6, 2, 3, TRACE>(s.llu, s.dllu, mp, s.lll, s.dlll, mp, tr, 2);
  joint_step<6, 6, 2, 3, TRACE>(s.rlu, s.drlu, mp, s.rll, s.drll, mp, tr, 3);
  if (s.post) {
#pragma unroll 1
    for (int k = 0; k < S.n_props; k++) prop_step<ROUGH>(s, mp, mb, dt, S, col, k, ter);
  }
  integrate(s.lll, s.dlll, dt, adx, ady);
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    if ((q == 0) == s.post) {
      floor_pairs<6, TRACE, 1, ROUGH>(s.lll, s.dlll, mp, s.clll, tr, 1, 0, ter);
      part_vs_props(s.lll, s.dlll, mp, S, col);
    } else {
      resolve_pair<6, 6, false, TRACE, 1>(s.lll, s.dlll, mp, s.llu, s.dllu, mp, s.clll, tr, 0, 0);
    }
  }
  integrate(s.llu, s.dllu, dt, adx, ady);
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    if ((q == 0) == s.post) {
      floor_pairs<6, TRACE, 1, ROUGH>(s.llu, s.dllu, mp, s.cllu, tr, 3, 0, ter);
      part_vs_props(s.llu, s.dllu, mp, S, col);
    } else {
      resolve_pair<6, 6, false, TRACE, 1>(s.llu, s.dllu, mp, s.lll, s.dlll, mp, s.cllu, tr, 2, 0);
    }
  }
  integrate(s.body, s.dbody, dt, adx, ady);
  floor_pairs<5, TRACE, 1, ROUGH>(s.body, s.dbody, mb, s.cbody, tr, 4, 0, ter);
  part_vs_props(s.body, s.dbody, mb, S, col);
  integrate(s.rll, s.drll, dt, adx, ady);
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    if ((q == 0) == s.post) {
      floor_pairs<6, TRACE, 1, ROUGH>(s.rll, s.drll, mp, s.crll, tr, 6, 0, ter);
      part_vs_props(s.rll, s.drll, mp, S, col);
    } else {
      resolve_pair<6, 6, false, TRACE, 1>(s.rll, s.drll, mp, s.rlu, s.drlu, mp, s.crll, tr, 5, 0);
    }
  }
  integrate(s.rlu, s.drlu, dt, adx, ady);
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    if ((q == 0) == s.post) {
      floor_pairs<6, TRACE, 1, ROUGH>(s.rlu, s.drlu, mp, s.crlu, tr, 8, 0, ter);
      part_vs_props(s.rlu, s.drlu, mp, S, col);
    } else {
      resolve_pair<6, 6, false, TRACE, 1>(s.rlu, s.drlu, mp, s.rll, s.drll, mp, s.crlu, tr, 7, 0);
    }
  }
  if (!s.post) {
#pragma unroll 1
    for (int k = 0; k < S.n_props; k++) prop_step<ROUGH>(s, mp, mb, dt, S, col, k, ter);
  }
}

// the one-lane env-step kernel with props: k_env_step's frame loop (env_frames, wk_env_lane.h,
// L = 1, no pacing, no counters) over substep_scene; its own part is the props -- A.props holds
// [n][S.pstride] prop state, staged in LDS for the launch (with the boxes) and written back
template <bool POLICY, bool RECORD, bool TRACE, bool ROUGH = false>
__global__ __launch_bounds__(64) void k_env_scene(EnvParams P, StepArgs A, SceneDev S) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = P.n_env;
  __shared__ float pl[(SCENE_FIELDS + 4 * SCENE_MAX_PROPS) * 64];  // state, then the boxes
  __shared__ float ter_lds[ROUGH ? 11 * 64 : 1];  // RoughFloor heights [draw][lane]
  if (e >= n) return;  // no barriers below: each lane touches only its own column
  float* col = pl + threadIdx.x;
  float* const ter = ter_lds + (ROUGH ? threadIdx.x : 0);
  if constexpr (ROUGH) {
#pragma unroll 1
    for (int i = 0; i < 11; i++)
      ter[i * 64] = 800.0f + (float)terrain_draw(P.seed, (uint32_t)(P.env_offset + e), i);
  }
  const float* pin = A.props + (size_t)e * S.pstride;
#pragma unroll 1
  for (int f = 0; f < S.pstride; f++) col[64 * f] = pin[f];
#pragma unroll 1
  for (int k = 0; k < S.n_props; k++) box_refresh(scene_prop(S, col, k));
  EnvState s;
  load_state(s, A.st, e, n);
  const float dx = A.dxoff[e];
  const StepConsts C = step_consts(P, A.mat[e]);
  uint32_t t = A.rng_t[e];
  uint32_t fault = 0;
  env_frames<POLICY, RECORD, TRACE, 1, false, false>(
      P, A, s, e, 0, dx, nullptr, t, fault, nullptr, [&](PairTraceDev* tr) __attribute__((always_inline)) {
        substep_scene<TRACE, ROUGH>(s, C.mp, C.mb, C.dt, C.adx, C.ady, tr, S, col, ter);
      });
  store_state(s, A.st, e, n);
  float* pout = A.props + (size_t)e * S.pstride;
#pragma unroll 1
  for (int f = 0; f < S.pstride; f++) pout[f] = col[64 * f];
  A.rng_t[e] = t;
  if (A.fault_out) A.fault_out[e] |= fault;
}

// host side: k_env_scene is instantiated where these are
template <bool ROUGH>
static void scene_given(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S, hipStream_t s) {
  dim3 blk(64), grd((unsigned)((P.n_env + 63) / 64));
  if (mode == 0) hipLaunchKernelGGL((k_env_scene<false, false, false, ROUGH>), grd, blk, 0, s, P, A, S);
  else hipLaunchKernelGGL((k_env_scene<false, false, true, ROUGH>), grd, blk, 0, s, P, A, S);
}
template <bool ROUGH>
static void scene_policy(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S, hipStream_t s) {
  dim3 blk(64), grd((unsigned)((P.n_env + 63) / 64));
  if (mode == 2) hipLaunchKernelGGL((k_env_scene<true, false, false, ROUGH>), grd, blk, 0, s, P, A, S);
  else hipLaunchKernelGGL((k_env_scene<true, true, false, ROUGH>), grd, blk, 0, s, P, A, S);
}
}  // namespace wk
