// sums_check.cpp -- the host arithmetic on wk_ppo_sums without a device (csrc/wk_sums.cpp): the
// fold step's order and its rmax rule, and the two divisions on the records they branch on -- no
// rows, a flat Var(ret), a NaN sum, no ratio.  Plain host C++ with its own main, so it can be built
// with -fsanitize=address,undefined and run as it is (tests/test_sums_binding.py does).
// Prints "sums_check ok" and returns 0, or the failed check and 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ppo-bipedalwalker_amd/csrc/wk_sums.cpp"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static wk_ppo_sums zero() {
  wk_ppo_sums s;
  memset(&s, 0, sizeof s);
  s.rmax = -std::numeric_limits<double>::infinity();
  return s;
}

static wk_ppo_sums plain() {
  wk_ppo_sums s = zero();
  s.rows = 8; s.skipped = 1; s.clipped = 5;
  s.kl = 0.25; s.k1 = -0.5; s.surr = 3.0;
  s.sr = 16.0; s.srr = 40.0; s.se = 1.0; s.see = 2.0;
  s.rmax = 1.75; s.term = -6.0; s.zz = 30.0;
  return s;
}

static wk_ppo_stats stats_of(const wk_ppo_sums& s) {
  wk_ppo_stats o;
  memset(&o, 0x5A, sizeof o);
  wk_ppo_stats_from_sums(&s, &o);
  return o;
}

static wk_log_std_grad grad_of(const wk_ppo_sums& s, float coef) {
  wk_log_std_grad g;
  memset(&g, 0x5A, sizeof g);
  wk_log_std_grad_from_sums(&s, coef, &g);
  return g;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(sizeof(wk_ppo_sums) == 13 * 8 && WK_COMM_RECORD_WORDS == 16);

  {  // the divisions on an exact record
    const wk_ppo_stats o = stats_of(plain());
    CHECK(o.samples == 8 && o.skipped == 1 && o.epochs_run == 0 && o.stopped_early == 0);
    CHECK(o.kl == 0.25 / 32 && o.kl_k1 == -0.5 / 32 && o.clip_fraction == 5.0 / 32 && o.ratio_max == 1.75);
    CHECK(o.surrogate == 3.0 / 32 && o.value_loss == 0.25);
    CHECK(o.explained_variance == 1.0 - (0.25 - 1.0 / 64));
    const wk_log_std_grad g = grad_of(plain(), 0.5f);
    CHECK(g.samples == 8 && g.skipped == 1 && g.grad_surrogate == 6.0 / 32 && g.grad == 6.0 / 32 - 0.5);
    CHECK(g.z2_mean == 30.0 / 32);
  }
  {  // no rows: every mean and the largest ratio are NaN
    const wk_ppo_stats o = stats_of(zero());
    CHECK(o.samples == 0 && std::isnan(o.kl) && std::isnan(o.kl_k1) && std::isnan(o.clip_fraction));
    CHECK(std::isnan(o.ratio_max) && std::isnan(o.surrogate) && std::isnan(o.value_loss));
    CHECK(std::isnan(o.explained_variance));
    const wk_log_std_grad g = grad_of(zero(), 0.01f);
    CHECK(g.samples == 0 && std::isnan(g.grad_surrogate) && std::isnan(g.grad) && std::isnan(g.z2_mean));
  }
  {  // a constant return, a NaN sum of squares, no counted ratio
    wk_ppo_sums s = plain();
    s.sr = 24.0; s.srr = 72.0;
    CHECK(std::isnan(stats_of(s).explained_variance) && stats_of(s).value_loss == 0.25);
    s = plain();
    s.srr = nan;
    CHECK(std::isnan(stats_of(s).explained_variance) && stats_of(s).kl == 0.25 / 32);
    s = plain();
    s.rmax = -inf;
    CHECK(stats_of(s).ratio_max == -inf);
    s.term = inf; s.zz = inf;
    CHECK(grad_of(s, 0.0f).grad == -inf && grad_of(s, 0.0f).z2_mean == inf);
  }
  {  // the fold: integers add, doubles add in the order given, rmax keeps a NaN from either side
    wk_ppo_sums a = zero(), b = zero(), c = zero();
    a.rows = 3; a.kl = 1e16; a.rmax = 1.5;
    b.rows = 5; b.kl = 1.0; b.rmax = 2.5;
    c.rows = 7; c.kl = 1.0; c.rmax = 0.5;
    wk_ppo_sums left = a;
    wk_ppo_sums_add(&left, &b);
    wk_ppo_sums_add(&left, &c);
    wk_ppo_sums bc = b, right = a;
    wk_ppo_sums_add(&bc, &c);
    wk_ppo_sums_add(&right, &bc);
    CHECK(left.kl == 1e16 && right.kl == 1e16 + 2.0 && left.rows == 15 && right.rows == 15);
    CHECK(left.rmax == 2.5 && right.rmax == 2.5);
    wk_ppo_sums n1 = zero(), five = zero();
    n1.rmax = nan; five.rmax = 5.0;
    wk_ppo_sums x = n1, y = five;
    wk_ppo_sums_add(&x, &five);
    wk_ppo_sums_add(&y, &n1);
    CHECK(std::isnan(x.rmax) && std::isnan(y.rmax));
    wk_ppo_sums u = plain(), z = zero();
    wk_ppo_sums_add(&u, &z);
    const wk_ppo_sums p = plain();
    CHECK(memcmp(&u, &p, sizeof u) == 0);
    std::vector<wk_ppo_sums> many(64, plain());  // a heap array folded in place
    for (size_t i = 1; i < many.size(); i++) wk_ppo_sums_add(&many[0], &many[i]);
    CHECK(many[0].rows == 8 * 64 && many[0].zz == 30.0 * 64 && many[0].rmax == 1.75);
  }
  // NULLs are ignored
  wk_ppo_sums s = plain();
  wk_ppo_stats o;
  wk_log_std_grad g;
  wk_ppo_sums_add(nullptr, &s);
  wk_ppo_sums_add(&s, nullptr);
  wk_ppo_stats_from_sums(nullptr, &o);
  wk_ppo_stats_from_sums(&s, nullptr);
  wk_log_std_grad_from_sums(nullptr, 0.0f, &g);
  wk_log_std_grad_from_sums(&s, 0.0f, nullptr);
  if (failures) return 1;
  printf("sums_check ok\n");
  return 0;
}
