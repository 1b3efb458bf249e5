"""CPU: sogm_det::atan2 and sogm_det::sin (include/sogm_detmath.h; the trajectory server's heading and the camera poses
built from it) against libm: atan2 within 4 ulp over 400 000 random pairs of magnitudes 1e-12 .. 1e12 (the bound the
project accepts for acos and log), exact on the axes with C's signs, odd in y bit for bit; sin within 2 eps as cos is.  The
Python restatement the trajectory server's fixture is generated with (tests/golden/make_traj_server_fixture.py) must give
the same bits."""
import importlib.util
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include "%s/include/sogm_detmath.h"
static double ulp(double a, double b) { if (a == b) return 0; double u = std::nextafter(std::fabs(b), INFINITY) - std::fabs(b); return std::fabs(a - b) / u; }
static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
int main() {
  std::mt19937_64 g(7); std::uniform_real_distribution<double> U(-1, 1);
  double ma = 0, ms = 0;
  for (int i = 0; i < 400000; i++) {
    const double y = U(g) * std::pow(10.0, U(g) * 12), x = U(g) * std::pow(10.0, U(g) * 12);
    const double a = sogm_det::atan2(y, x);
    ma = std::max(ma, ulp(a, std::atan2(y, x)));
    if (!same(a, -sogm_det::atan2(-y, x))) return 2;                       // odd in y
    const double t = U(g) * 7; ms = std::max(ms, std::fabs(sogm_det::sin(t) - std::sin(t)) / 2.220446049250313e-16);
    if (!same(sogm_det::sin(-t), -sogm_det::sin(t))) return 5;
    if (i < 64) std::printf("%%a %%a %%a\n", y, x, a);                        // for the Python restatement
  }
  // the unit circle's neighbourhood too: directions are what the server feeds it
  for (int i = 0; i < 400000; i++) {
    const double y = U(g), x = U(g);
    ma = std::max(ma, ulp(sogm_det::atan2(y, x), std::atan2(y, x)));
  }
  // axes and diagonals, with C's signs
  const double P = 3.141592653589793, H = 1.5707963267948966, Q = 0.7853981633974483;
  const double ax[][3] = {{0.0, 1.0, 0.0}, {-0.0, 1.0, -0.0}, {0.0, 0.0, 0.0}, {-0.0, 0.0, -0.0}, {0.0, -0.0, P}, {-0.0, -0.0, -P},
                          {0.0, -2.5, P}, {-0.0, -2.5, -P}, {3.0, 0.0, H}, {3.0, -0.0, H}, {-3.0, 0.0, -H}, {1e-300, 0.0, H},
                          {2.0, 2.0, Q}, {-2.0, 2.0, -Q}, {1e12, 0.0, H}, {0.0, 1e-12, 0.0}};
  for (auto &r : ax) if (!same(sogm_det::atan2(r[0], r[1]), r[2])) return 3;
  if (sogm_det::sin(0.0) != 0.0) return 4;
  std::printf("max %%.3f %%.3f\n", ma, ms);
  return 0;
}
'''


def test_atan2_and_sin_accuracy(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(SRC % ROOT)
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    atan2_ulp, sin_eps = map(float, lines[-1].split()[1:])
    print("atan2 max ulp", atan2_ulp, "sin max eps", sin_eps)
    assert atan2_ulp <= 4 and sin_eps <= 2
    # the fixture generator's restatement: the same bits
    spec = importlib.util.spec_from_file_location("make_traj_server_fixture",
                                                  os.path.join(ROOT, "tests", "golden", "make_traj_server_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert len(lines) == 65
    for line in lines[:-1]:
        y, x, a = (float.fromhex(v) for v in line.split())
        assert struct.pack("<d", gen.det_atan2(y, x)) == struct.pack("<d", a), (y, x)
