// host_selftest_mixed.cpp — native self-test of OP_RUN_MIXED's host paths through the C ABI, built
// under AddressSanitizer+UBSan (`make -C csrc asan-mixed`) or ThreadSanitizer (`make -C csrc
// tsan-mixed`) from the sanitised objects of `asan` / `tsan`.  One lane-template shape (WW(2,2)) and
// one runtime shape (WW(3,3)): the fused operator against the same counter schedule built from
// OP_CLASSIFY / OP_RUN_FIXPOINT / OP_TRAIN through srnn_run on compacted tables, bit for bit -- the
// final table, classes, step counts, losses and the recorded trajectory.
#include "../srnn_abi.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

static void run(int op, const SrnnCfg& c, const SrnnArgs& a) {
  int r = srnn_run(op, &c, &a);
  if (r != 0) {
    std::fprintf(stderr, "srnn_run(%d) = %d: %s\n", op, r, srnn_last_error());
    ++g_fail;
  }
}

static SrnnCfg ww(int w, int d) {
  SrnnCfg c{};
  c.kind = 0, c.width = w, c.depth = d;
  c.p = 4 * w + (d - 1) * w * w + w, c.pp = (c.p + 3) & ~3;
  return c;
}

struct Out {
  std::vector<float> W, loss, traj;
  std::vector<int8_t> cls;
  std::vector<int32_t> nsteps;
};

static SrnnArgs base_args(int64_t n, uint32_t ctr) {
  SrnnArgs a{};
  a.n = n, a.seed = 11, a.ctr = ctr, a.dev = 0, a.lr = 0.01f, a.eps = 1e-4f;
  return a;
}

static Out fused(const SrnnCfg& c, const std::vector<float>& W0, const std::vector<int64_t>& uid, int K, int T,
                 int early, uint32_t c0) {
  const int64_t n = (int64_t)uid.size();
  Out o;
  o.W = W0;
  o.loss.assign((size_t)n, -1.f), o.cls.assign((size_t)n, -1), o.nsteps.assign((size_t)n, -1);
  o.traj.assign((size_t)((K + 1) * n * c.pp), 0.f);
  SrnnArgs a = base_args(n, c0);
  a.steps = K, a.epochs = T, a.early_exit = early, a.flags = SRNN_F_SHUFFLE | SRNN_F_FIX_SEC;
  a.W = o.W.data(), a.uid = uid.data(), a.cls = o.cls.data(), a.nsteps = o.nsteps.data();
  a.loss = o.loss.data(), a.traj = o.traj.data();
  run(OP_RUN_MIXED, c, a);
  return o;
}

static Out sequence(const SrnnCfg& c, const std::vector<float>& W0, const std::vector<int64_t>& uid, int K, int T,
                    int early, uint32_t c0) {
  const int64_t n = (int64_t)uid.size();
  const int PP = c.pp;
  Out o;
  o.W = W0;
  o.loss.assign((size_t)n, 0.f), o.cls.assign((size_t)n, -1), o.nsteps.assign((size_t)n, 0);
  o.traj.assign((size_t)((K + 1) * n * PP), 0.f);
  std::memcpy(o.traj.data(), W0.data(), (size_t)(n * PP) * sizeof(float));
  std::vector<int64_t> rows((size_t)n);
  for (int64_t i = 0; i < n; ++i) rows[(size_t)i] = i;
  for (int s = 0; s < K && !rows.empty(); ++s) {
    const uint32_t cs = c0 + (uint32_t)s * (uint32_t)(T + 2);
    auto gather = [&](std::vector<float>& sub, std::vector<int64_t>& su) {
      sub.resize(rows.size() * (size_t)PP), su.resize(rows.size());
      for (size_t q = 0; q < rows.size(); ++q) {
        std::memcpy(&sub[q * (size_t)PP], &o.W[(size_t)(rows[q] * PP)], (size_t)PP * sizeof(float));
        su[q] = uid[(size_t)rows[q]];
      }
    };
    std::vector<float> sub, sl;
    std::vector<int64_t> su;
    std::vector<int8_t> k;
    gather(sub, su);
    if (s > 0 || early == 1) {
      k.assign(rows.size(), -1);
      SrnnArgs a = base_args((int64_t)rows.size(), cs);
      a.W = sub.data(), a.uid = su.data(), a.cls = k.data();
      run(OP_CLASSIFY, c, a);
      std::vector<int64_t> keep;
      for (size_t q = 0; q < rows.size(); ++q)
        if (k[q] == 4) keep.push_back(rows[q]);
      rows.swap(keep);
      if (rows.empty()) break;
      gather(sub, su);
    }
    SrnnArgs f = base_args((int64_t)rows.size(), cs);
    f.W = sub.data(), f.uid = su.data(), f.steps = 1, f.early_exit = 0;
    run(OP_RUN_FIXPOINT, c, f);
    if (T > 0) {
      sl.assign(rows.size(), 0.f);
      SrnnArgs t = base_args((int64_t)rows.size(), cs + 1u);
      t.W = sub.data(), t.uid = su.data(), t.epochs = T, t.flags = SRNN_F_SHUFFLE, t.loss = sl.data();
      run(OP_TRAIN, c, t);
    }
    for (size_t q = 0; q < rows.size(); ++q) {
      const int64_t r = rows[q];
      std::memcpy(&o.W[(size_t)(r * PP)], &sub[q * (size_t)PP], (size_t)PP * sizeof(float));
      std::memcpy(&o.traj[(size_t)(((int64_t)(s + 1) * n + r) * PP)], &sub[q * (size_t)PP], (size_t)PP * sizeof(float));
      o.nsteps[(size_t)r] += 1;
      if (T > 0) o.loss[(size_t)r] = sl[q];
    }
  }
  SrnnArgs a = base_args(n, c0 + (uint32_t)K * (uint32_t)(T + 2));
  a.W = o.W.data(), a.uid = uid.data(), a.cls = o.cls.data(), a.flags = SRNN_F_FIX_SEC;
  run(OP_CLASSIFY, c, a);
  return o;
}

static bool same(const std::vector<float>& x, const std::vector<float>& y) {
  return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(float)) == 0;
}

static void mixed_case(const SrnnCfg& c, int64_t n, int K, int T, int early) {
  std::vector<float> W0((size_t)(n * c.pp), 0.f);
  std::vector<int64_t> uid((size_t)n);
  for (int64_t i = 0; i < n; ++i) uid[(size_t)i] = i + 7;
  SrnnArgs a = base_args(n, 0);
  a.W = W0.data(), a.uid = uid.data();
  run(OP_INIT, c, a);
  // a zero row (a fixpoint from the start) and a row holding an infinity (divergent from the start)
  for (int k = 0; k < c.pp; ++k) W0[(size_t)k] = 0.f;
  if (n > 1) W0[(size_t)c.pp] = INFINITY;
  const Out f = fused(c, W0, uid, K, T, early, 7), s = sequence(c, W0, uid, K, T, early, 7);
  CHECK(same(f.W, s.W));
  CHECK(same(f.loss, s.loss));
  CHECK(same(f.traj, s.traj));
  CHECK(f.cls == s.cls);
  CHECK(f.nsteps == s.nsteps);
  CHECK(f.nsteps[0] == (early == 1 ? 0 : 1));
  int moved = 0;
  for (int64_t i = 0; i < n; ++i) moved += f.nsteps[(size_t)i] >= 2;
  CHECK(n < 8 || moved > 0);
}

int main() {
  if (srnn_abi_version() != 32) {
    std::fprintf(stderr, "ABI %d\n", srnn_abi_version());
    return 2;
  }
  const SrnnCfg shapes[2] = {ww(2, 2), ww(3, 3)};  // lane template, runtime shape
  for (const SrnnCfg& c : shapes) {
    CHECK(srnn_supports(&c, OP_RUN_MIXED, 0) == 1);
    CHECK(srnn_train_form(&c, 0) == 1);
    for (int early = 1; early <= 2; ++early) {
      mixed_case(c, 300, 4, 3, early);  // over the thread pool's threshold
      mixed_case(c, 65, 3, 0, early);
      mixed_case(c, 1, 2, 1, early);
    }
  }
  if (g_fail) {
    std::fprintf(stderr, "host_selftest_mixed: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("host_selftest_mixed: ok\n");
  return 0;
}
