// Compiles against host/sogm_facade.hpp's Links::setNoise / sent / sentShift / auditBelief / belief.  Without a GPU: the default
// noise is all zero, the default belief parameters are the header's, bad parameters are refused with the rule's text.  With one:
// three receivers on perfect links — zero noise hands every receiver the table byte for byte and the audit finds every sample
// in bin 0; a localisation bias moves every control point of a message by its row's shift (the rule's one add, redone here)
// and the audit's largest q is round(|shift|^2 * 1e6) within one.  Prints "links noise facade ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sogm_facade.hpp"

static int fails = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);  \
      ++fails;                                                 \
    }                                                          \
  } while (0)

static std::vector<SogmTrajRecord> table_of(int n) {
  std::vector<SogmTrajRecord> t((size_t)n);
  for (int j = 0; j < n; ++j) {
    std::memset(&t[j], 0, sizeof(SogmTrajRecord));
    t[j].drone_id   = j;
    t[j].n_pieces   = 1 + j;
    t[j].time_start = 10.0;
    for (int k = 0; k < SOGM_MAX_PIECES; ++k) t[j].duration[k] = 0.5;
    for (int i = 0; i < SOGM_MAX_PIECES * 15; ++i) t[j].cpts[i] = j * 10.0 + i * 0.125;
  }
  return t;
}

int main() {
  static_assert(sizeof(SogmTrajNoise) == 56 && sizeof(SogmBeliefParams) == 56 && SOGM_BELIEF_COUNTERS == 12, "layout");
  const SogmTrajNoise quiet = sogm_host::Links::defaultNoise();
  const SogmTrajNoise zero{};
  EXPECT(std::memcmp(&quiet, &zero, sizeof(zero)) == 0);
  const SogmBeliefParams bp = sogm_host::Links::defaultBeliefParams();
  EXPECT(bp.n_samples == 8 && bp.dt_sample == 0.2 && bp.edges[0] == 0.05 && bp.edges[4] == 1.0);
  SogmTrajRecord *fake_rec = reinterpret_cast<SogmTrajRecord *>(0x1000);
  SogmTrajNoise   bad      = quiet;
  bad.sigma_track          = -1.0;
  EXPECT(sogm_traj_noise(&bad, 0, fake_rec, 3, fake_rec, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_traj_noise") && std::strstr(sogm_last_error(), "sigma_track"));
  SogmBeliefParams bad_bp = bp;
  bad_bp.n_samples        = 17;
  EXPECT(sogm_belief_audit(&bad_bp, fake_rec, fake_rec, reinterpret_cast<double *>(0x1000), 3, 0, 3,
                           reinterpret_cast<int64_t *>(0x1000), nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_belief_audit") && std::strstr(sogm_last_error(), "n_samples"));
  if (sogm_device_count() == 0) {
    EXPECT(sogm_traj_noise(&quiet, 0, fake_rec, 3, fake_rec, nullptr, nullptr) == SOGM_ERR_NO_DEVICE);
  } else {
    const int                         n = 3;
    const auto                        t = table_of(n);
    sogm_host::DevBuf<SogmTrajRecord> dev((size_t)n);
    sogm_host::DevBuf<double>         t_now((size_t)n);
    const std::vector<double>         now((size_t)n, 10.0);
    dev.put(t.data(), t.size());
    t_now.put(now.data(), now.size());
    std::vector<SogmTrajRecord> got((size_t)n * n);
    {
      sogm_host::Links l(sogm_host::Links::defaultParams(), n, 0, n);
      {
        const auto c0 = l.belief();
        bool       zero = c0.size() == (size_t)n * SOGM_BELIEF_COUNTERS;
        for (int64_t v : c0) zero = zero && v == 0;
        EXPECT(zero);
      }
      l.setNoise(quiet);
      l.deliver(0, dev.data(), nullptr);
      l.auditBelief(bp, dev.data(), t_now.data());
      (void)hipDeviceSynchronize();
      (void)hipMemcpy(got.data(), l.views(), got.size() * sizeof(SogmTrajRecord), hipMemcpyDeviceToHost);
      for (int a = 0; a < n; ++a) EXPECT(std::memcmp(&got[(size_t)a * n], t.data(), sizeof(SogmTrajRecord) * n) == 0);
      const auto c = l.belief();
      EXPECT(c.size() == (size_t)n * SOGM_BELIEF_COUNTERS);
      for (int a = 0; a < n; ++a) {
        const int64_t *r = &c[(size_t)a * SOGM_BELIEF_COUNTERS];
        EXPECT(r[0] == n - 1 && r[1] == 0 && r[2] == 0 && r[3] == 8 * (n - 1) && r[4] == r[3] && r[10] == 0 && r[11] == 0);
      }
    }
    {
      SogmTrajNoise noise = quiet;
      noise.seed          = 0x5067;
      noise.sigma_loc[0] = noise.sigma_loc[1] = noise.sigma_loc[2] = 0.1;
      sogm_host::Links l(sogm_host::Links::defaultParams(), n, 0, n);
      l.setNoise(noise);
      l.deliver(0, dev.data(), nullptr);
      l.auditBelief(bp, dev.data(), t_now.data());
      l.auditBelief(bp, dev.data(), t_now.data());
      (void)hipDeviceSynchronize();
      std::vector<double> shift((size_t)n * 4);
      (void)hipMemcpy(shift.data(), l.sentShift(), shift.size() * sizeof(double), hipMemcpyDeviceToHost);
      (void)hipMemcpy(got.data(), l.views(), got.size() * sizeof(SogmTrajRecord), hipMemcpyDeviceToHost);
      for (int a = 0; a < n; ++a)
        for (int j = 0; j < n; ++j) {
          const SogmTrajRecord &r = got[(size_t)a * n + j];
          EXPECT(r.n_pieces == t[j].n_pieces && r.time_start == t[j].time_start && shift[(size_t)j * 4 + 3] == 0.0);
          bool same = true;
          for (int i = 0; i < SOGM_MAX_PIECES * 15; ++i) {
            const volatile double want = i < 15 * t[j].n_pieces ? t[j].cpts[i] + shift[(size_t)j * 4 + i % 3] : t[j].cpts[i];
            same = same && r.cpts[i] == want;
          }
          EXPECT(same);
        }
      const auto c = l.belief();
      for (int a = 0; a < n; ++a) {
        const int64_t *r     = &c[(size_t)a * SOGM_BELIEF_COUNTERS];
        int64_t        worst = 0;
        for (int j = 0; j < n; ++j) {
          if (j == a) continue;
          const double *s = &shift[(size_t)j * 4];
          EXPECT(s[0] != 0.0 && s[1] != 0.0 && s[2] != 0.0);
          const int64_t q = (int64_t)std::floor((s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) * 1e6 + 0.5);
          worst           = q > worst ? q : worst;
        }
        EXPECT(r[0] == 2 * (n - 1) && r[3] == 2 * 8 * (n - 1) && r[11] >= worst - 1 && r[11] <= worst + 1);   // two calls
      }
    }
  }
  if (fails) return 1;
  std::printf("links noise facade ok\n");
  return 0;
}
