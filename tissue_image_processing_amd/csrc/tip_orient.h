// tip_orient.h -- the exact orientation predicate of the hull code (tip_hull.hip), compiled for the device and for the host from
// the same text: the kernels, the host-array forms' checks and tip_sensory_region_host all decide with orient() and nothing else,
// so no tolerance enters a hull or an inside / outside answer.  DESIGN.md 5.13 has the argument.
//
//   orient(a, b, p) = the sign (-1, 0, +1) of (b - a) x (p - a) = (bx - ax)(py - ay) - (by - ay)(px - ax) over the reals:
//   +1 when p lies strictly to the left of the directed line a -> b, 0 when the three are collinear (or two coincide).
//
// Stage A, the floating filter (Shewchuk 1997, orient2d's first stage): the two products and their difference as rounded
// operations; the difference's sign is the exact one when |det| > (3 + 16 eps) eps (|left| + |right|), eps = 2^-53 -- the
// certificate, as tip_order.hip words its empty-circle one: every operation is a single explicitly rounded one
// (-ffp-contract=off is the build's rule; nothing here may be fused behind the bound's back).
// Stage B, when the filter cannot decide: the determinant multiplied out,
//   bx py - bx ay - ax py - by px + by ax + ay px      (ax ay cancels),
// each product as an error-free pair (two_product: p = fl(a b), e = fma(a, b, -p), the one place a fused operation is WANTED
// and therefore written out), the twelve terms summed into a non-overlapping expansion with two_sum (Knuth's six operations,
// grow-expansion); the sign is the sign of the expansion's largest non-zero component.  Exact unless a product overflows or
// is subnormal -- coordinates are pixel positions here; |coordinate| < 2^500 and, where non-zero, > 2^-500 is ample.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TIP_HD __host__ __device__
#else
#define TIP_HD
#endif

namespace tip {

TIP_HD inline void two_sum(double a, double b, double &s, double &e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

TIP_HD inline void two_product(double a, double b, double &p, double &e)
{
    p = a * b;
    e = fma(a, b, -p);
}

// e[0 .. m) non-overlapping, increasing magnitude; adds b, leaves m + 1 components (Shewchuk's Grow-Expansion)
template <int M>
TIP_HD inline void grow_expansion(double (&e)[M], int m, double b)
{
    double q = b;
    for (int i = 0; i < m; ++i) two_sum(q, e[i], q, e[i]);
    e[m] = q;
}

TIP_HD inline int orient_exact(double ax, double ay, double bx, double by, double px, double py)
{
    const double f[6][2] = {{bx, py}, {-bx, ay}, {-ax, py}, {-by, px}, {by, ax}, {ay, px}};
    double e[12];
    int m = 0;
    for (int k = 0; k < 6; ++k) {
        double p, err;
        two_product(f[k][0], f[k][1], p, err);
        grow_expansion(e, m++, err);
        grow_expansion(e, m++, p);
    }
    for (int i = 11; i >= 0; --i)
        if (e[i] != 0.0) return e[i] > 0.0 ? 1 : -1;
    return 0;
}

TIP_HD inline int orient(double ax, double ay, double bx, double by, double px, double py)
{
    const double left = (bx - ax) * (py - ay), right = (by - ay) * (px - ax);
    const double det = left - right;
    const double bound = 3.3306690738754716e-16 * (fabs(left) + fabs(right));      // (3 + 16 eps) eps, eps = 2^-53
    if (det > bound) return 1;
    if (-det > bound) return -1;
    return orient_exact(ax, ay, bx, by, px, py);
}

// (x, y, index) in lexicographic order: the hull's sort key and its start vertex
TIP_HD inline bool lex_less(double ax, double ay, int ai, double bx, double by, int bi)
{
    return ax < bx || (ax == bx && (ay < by || (ay == by && ai < bi)));
}

}  // namespace tip
