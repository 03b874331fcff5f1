/* wk_sincos_small.h -- sin / cos of a small angle in double, for the rotation's
 * (float)Math.Sin/Cos((double)angle) (XNA CreateRotationZ, Skeleton.Rotate Skeleton.cs:89-97).
 * Taylor series in Horner form with explicit FMAs, valid for |x| <= 0.25 (truncation
 * below 1e-20 relative).  Shared by the device code and the host-side exhaustive check
 * (tests/cpp/sincos_small_check.c), which proves (float) of it equals (float) of the C
 * library's sin / cos for every float in that range. */
#ifndef WK_SINCOS_SMALL_H
#define WK_SINCOS_SMALL_H
#ifdef __HIP__
#define WK_SC_FN __host__ __device__ __forceinline__
#else
#define WK_SC_FN static inline
#include <math.h>
#endif

/* One Horner step p * x2 + k with a uniform constant k.  On the device the constant is a scalar
 * operand of a three-address v_fma_f64: left to itself the compiler keeps the thirteen
 * coefficients in VGPR pairs and uses the two-address v_fmac_f64, which first copies each
 * coefficient into the accumulator (17 register copies per rotation and about 20 VGPRs held
 * across the substep loop).  The same single FMA, the same operands: bit-identical
 * (tests/cpp/sincos_dev_check.hip).  The host build keeps the plain form, and so does a device
 * build that defines WK_SC_PLAIN_FMA (the rough-floor side kernels, wk_env_side_rough.hip). */
#if defined(__HIP_DEVICE_COMPILE__) && defined(__AMDGCN__) && !defined(WK_SC_PLAIN_FMA)
WK_SC_FN double wk_sc_step(double p, double x2, double k) {
  double r;
  __asm__("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(p), "v"(x2), "s"(k));
  return r;
}
/* the first step k0 * x2 + k1: two constants, one scalar (the instruction reads one scalar pair) */
WK_SC_FN double wk_sc_first(double k0, double x2, double k1) {
  double r;
  __asm__("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "s"(k0), "v"(x2), "v"(k1));
  return r;
}
/* The sine's chain ps and the cosine's chain pc are independent; their steps alternate so that
 * no step directly follows the one it reads (the compiler puts a wait state between an asm
 * statement and an instruction that reads its result).  Each chain is the sequence of FMAs of
 * the plain form below, on the same operands. */
WK_SC_FN void wk_sincos_small(double x, double* s, double* c) {
  const double x2 = x * x;
  double pc = -1.0 / 87178291200.0;                 /* -1/14! */
  double ps = 1.0 / 6227020800.0;                   /*  1/13! */
  pc = wk_sc_first(pc, x2, 1.0 / 479001600.0);      /*  1/12! */
  ps = wk_sc_first(ps, x2, -1.0 / 39916800.0);      /* -1/11! */
  pc = wk_sc_step(pc, x2, -1.0 / 3628800.0);        /* -1/10! */
  ps = wk_sc_step(ps, x2, 1.0 / 362880.0);          /*  1/9!  */
  pc = wk_sc_step(pc, x2, 1.0 / 40320.0);           /*  1/8!  */
  ps = wk_sc_step(ps, x2, -1.0 / 5040.0);           /* -1/7!  */
  pc = wk_sc_step(pc, x2, -1.0 / 720.0);            /* -1/6!  */
  ps = wk_sc_step(ps, x2, 1.0 / 120.0);             /*  1/5!  */
  pc = wk_sc_step(pc, x2, 1.0 / 24.0);              /*  1/4!  */
  ps = wk_sc_step(ps, x2, -1.0 / 6.0);              /* -1/3!  */
  pc = __builtin_fma(pc, x2, -0.5);                 /* -1/2!  (inline constants) */
  *s = __builtin_fma(x * x2, ps, x);
  *c = __builtin_fma(x2, pc, 1.0);
}
#else
WK_SC_FN void wk_sincos_small(double x, double* s, double* c) {
  const double x2 = x * x;
  double ps = 1.0 / 6227020800.0;                   /*  1/13! */
  ps = __builtin_fma(ps, x2, -1.0 / 39916800.0);    /* -1/11! */
  ps = __builtin_fma(ps, x2, 1.0 / 362880.0);       /*  1/9!  */
  ps = __builtin_fma(ps, x2, -1.0 / 5040.0);        /* -1/7!  */
  ps = __builtin_fma(ps, x2, 1.0 / 120.0);          /*  1/5!  */
  ps = __builtin_fma(ps, x2, -1.0 / 6.0);           /* -1/3!  */
  *s = __builtin_fma(x * x2, ps, x);
  double pc = -1.0 / 87178291200.0;                 /* -1/14! */
  pc = __builtin_fma(pc, x2, 1.0 / 479001600.0);    /*  1/12! */
  pc = __builtin_fma(pc, x2, -1.0 / 3628800.0);     /* -1/10! */
  pc = __builtin_fma(pc, x2, 1.0 / 40320.0);        /*  1/8!  */
  pc = __builtin_fma(pc, x2, -1.0 / 720.0);         /* -1/6!  */
  pc = __builtin_fma(pc, x2, 1.0 / 24.0);           /*  1/4!  */
  pc = __builtin_fma(pc, x2, -0.5);                 /* -1/2!  */
  *c = __builtin_fma(x2, pc, 1.0);
}
#endif
#endif
