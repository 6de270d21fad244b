// The launch that finishes clouds of at most 4096 points LDS-resident (see emd_resident.h).
#include "emd_resident.h"

namespace mvp {

template <int NMAX>
__global__ __launch_bounds__(kEmdThreads) void emd_resident_kernel(
    int b, int n, float *__restrict__ dist, int *assignment, float eps, int iters, char *scratch) {
  __shared__ ResShared<NMAX> sh;
  emd_resident_body<NMAX>(sh, (int)blockIdx.x, b, n, dist, assignment, eps, iters, scratch);
}

// Finishes the clouds emd_lean.hip's launch stopped for it (hand-over records with next_it != 0).
hipError_t emd_resident_launch(const EmdStep &s, EmdCall c) {
  void *args[] = {&c.b, &c.n, &c.dist, &c.assignment, &c.eps, &c.iters, &c.scratch};
  const void *kernel = nullptr;   // (no such instantiation: the launch fails)
  switch (s.resn) {
    case 2048: kernel = reinterpret_cast<const void *>(emd_resident_kernel<2048>); break;
    case 4096: kernel = reinterpret_cast<const void *>(emd_resident_kernel<4096>); break;
  }
  return emd_launch_step(kernel, s, args, c.stream);
}

}  // namespace mvp
