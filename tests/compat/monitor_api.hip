// t8gpu::hip::Monitor (include/t8gpu/backend/hip_fast.h) on a hand-made state: plain cells in fp64, Subgrid<4,4> cells in
// fp32, one broken cell each. Prints "monitor_api OK".
#include <t8gpu/backend/hip_fast.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(call)                                                                  \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess) {                                                          \
      std::printf("%s failed: %s\n", #call, hipGetErrorString(e_));                  \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

template<typename ft>
static int run(int cells_per_element, int dim, size_t elements) {
  const size_t    n = elements * cells_per_element;
  std::vector<ft> u(5 * n), vol(elements);
  double          mass = 0, smax = 0, rate = 0, rho_min = 1e300;
  for (size_t e = 0; e < elements; e++) vol[e] = static_cast<ft>(0.25 + 0.001 * static_cast<double>(e % 7));
  for (size_t i = 0; i < n; i++) {
    const double rho = 1.0 + 0.01 * static_cast<double>(i % 13), vx = 0.1 * static_cast<double>(i % 5), p = 1.0 + 0.02 * static_cast<double>(i % 3);
    u[i] = static_cast<ft>(rho), u[n + i] = static_cast<ft>(rho * vx), u[2 * n + i] = 0, u[3 * n + i] = 0;
    u[4 * n + i] = static_cast<ft>(p / 0.4 + 0.5 * rho * vx * vx);
  }
  u[4 * n + 3] = static_cast<ft>(NAN);   // one non-finite cell
  for (size_t i = 0; i < n; i++) {
    if (i == 3) continue;
    const double rho = u[i], mx = u[n + i], E = u[4 * n + i], v = static_cast<double>(vol[i / cells_per_element]) / cells_per_element;
    const double p = 0.4 * (E - 0.5 * mx * mx / rho), s = std::fabs(mx) / rho + std::sqrt(1.4 * p / rho);
    mass += v * rho;
    smax    = std::max(smax, s);
    rate    = std::max(rate, s / (dim == 2 ? std::sqrt(v) : std::cbrt(v)));
    rho_min = std::min(rho_min, rho);
  }
  ft *d_u = nullptr, *d_vol = nullptr;
  CHECK(hipMalloc(&d_u, sizeof(ft) * u.size()));
  CHECK(hipMalloc(&d_vol, sizeof(ft) * vol.size()));
  CHECK(hipMemcpy(d_u, u.data(), sizeof(ft) * u.size(), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_vol, vol.data(), sizeof(ft) * vol.size(), hipMemcpyHostToDevice));
  t8gpu::hip::Monitor        monitor;
  t8gpu::hip::Monitor::block b = monitor.run<ft>(n, cells_per_element, dim, t8gpu::hip::to_vars<ft>(d_u, n), d_vol);
  CHECK(hipFree(d_u));
  CHECK(hipFree(d_vol));
  auto close = [](double got, double want) { return std::fabs(got - want) <= 1e-12 * std::fabs(want); };
  const bool ok = close(b[0], mass) && close(b[7], smax) && close(b[8], rate) && b[9] == rho_min && b[11] == 1.0 && b[12] == 0.0 &&
                  b[13] == 0.0 && b[15] == 0.0;
  if (!ok) std::printf("mismatch (%d cells per element): mass %.17g / %.17g, max s %.17g / %.17g, rate %.17g / %.17g, min rho %.17g / %.17g, counts %g %g\n",
                       cells_per_element, b[0], mass, b[7], smax, b[8], rate, b[9], rho_min, b[11], b[12]);
  return ok ? 0 : 1;
}

int main() {
  if (run<double>(1, 3, 1001) || run<float>(16, 2, 300)) return 1;
  std::printf("monitor_api OK\n");
  return 0;
}
