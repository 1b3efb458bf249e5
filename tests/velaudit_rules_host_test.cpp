// Host build of csrc/sogm_velaudit.hpp (the body k_vel_audit calls, and the sequential form of the whole rule): reads cases
// from a file (or stdin), prints two lines per case.  One case (one agent) per line:
//   A ok range_len max_points n_codes has_codes tol (fp32 bits)
//     n_born  then n_born x { row[7] (fp32 bits)  src }
//     n_truth then n_truth x { label[4] (fp32 bits)  code }         n_truth >= min(range_len, max_points)
//   -> "R" + the 32 values of the row
//   -> "T" + the (n_codes + 2) * 6 values of the per-code table (nothing after "T" without codes)
// tests/test_velocity_audit_host.py holds the output to the numpy reading (tests/velocity_audit_reference.py).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sogm_velaudit.hpp"

static float f32(const std::string &h) {
  const uint32_t u = (uint32_t)std::stoul(h, nullptr, 16);
  float          f;
  std::memcpy(&f, &u, sizeof f);
  return f;
}

static int run(std::istream &in) {
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string        tag, h;
    ss >> tag;
    if (tag.empty()) continue;
    if (tag != "A") return 5;
    int       ok, max_points, n_codes, has_codes, n_born, n_truth;
    long long range_len;
    ss >> ok >> range_len >> max_points >> n_codes >> has_codes >> h;
    if (!ss || max_points < 1 || n_codes < 0) return 4;
    const float tol = f32(h);
    ss >> n_born;
    if (!ss || n_born < 0 || n_born > max_points) return 4;
    std::vector<float>   born((size_t)n_born * 7 + 1);
    std::vector<int32_t> src((size_t)n_born + 1);
    for (int k = 0; k < n_born; ++k) {
      for (int j = 0; j < 7; ++j) ss >> h, born[(size_t)k * 7 + j] = f32(h);
      ss >> src[k];
    }
    ss >> n_truth;
    const long long n_in = range_len < max_points ? range_len : max_points;
    if (!ss || n_truth < 0 || (long long)n_truth < n_in) return 6;
    std::vector<float>   truth((size_t)n_truth * 4 + 1);
    std::vector<int32_t> code((size_t)n_truth + 1);
    for (int i = 0; i < n_truth; ++i) {
      for (int j = 0; j < 4; ++j) ss >> h, truth[(size_t)i * 4 + j] = f32(h);
      ss >> code[i];
    }
    if (!ss) return 7;
    std::vector<uint32_t>  seen((size_t)(max_points + 31) / 32);
    std::vector<long long> row(sogm::VELROW_N, 0), table((size_t)(n_codes + 2) * sogm::VELCODE_COLS, 0);
    sogm::velaudit_agent(ok != 0, range_len, max_points, n_born, born.data(), src.data(), truth.data(),
                         has_codes ? code.data() : nullptr, n_codes, tol, seen.data(), row.data(),
                         has_codes ? table.data() : nullptr);
    std::printf("R");
    for (long long v : row) std::printf(" %lld", v);
    std::printf("\nT");
    if (has_codes)
      for (long long v : table) std::printf(" %lld", v);
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return run(std::cin);
  std::ifstream in(argv[1]);
  if (!in) return 3;
  return run(in);
}
