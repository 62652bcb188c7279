// what does a launch that finds the solve done cost?  K launches of a kernel that reads a flag and returns (the shape of the grid-wide Krylov kernels on a
// 27 x 25 x 21 bottom: 56 workgroups of 256 threads; and on a 75^3 bottom: 256 of 512), captured into a hipGraph and replayed, and launched one by one.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
__global__ void __launch_bounds__(1024) noop(const double *st, double *out) {
  if (st[0] != 0.0) return;
  out[blockIdx.x * blockDim.x + threadIdx.x] = 1.0;
}
int main() {
  double *st, *out;
  CHK(hipMalloc(&st, 256)); CHK(hipMalloc(&out, 8 * 256 * 1024));
  double one = 1.0;
  CHK(hipMemcpy(st, &one, 8, hipMemcpyHostToDevice));
  hipStream_t s; CHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipEvent_t a, b; CHK(hipEventCreate(&a)); CHK(hipEventCreate(&b));
  const int shapes[2][2] = { { 56, 256 }, { 256, 512 } };
  for (int q = 0; q < 2; q++) for (int K : { 300, 3000 }) {
    const dim3 G(shapes[q][0]), B(shapes[q][1]);
    hipGraph_t g; hipGraphExec_t ge;
    CHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int k = 0; k < K; k++) hipLaunchKernelGGL(noop, G, B, 0, s, st, out);
    CHK(hipStreamEndCapture(s, &g));
    CHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    CHK(hipGraphLaunch(ge, s)); CHK(hipStreamSynchronize(s));
    float best = 1e30f;
    for (int rep = 0; rep < 5; rep++) {
      CHK(hipEventRecord(a, s)); CHK(hipGraphLaunch(ge, s)); CHK(hipEventRecord(b, s)); CHK(hipStreamSynchronize(s));
      float ms; CHK(hipEventElapsedTime(&ms, a, b)); if (ms < best) best = ms;
    }
    float beste = 1e30f;
    for (int rep = 0; rep < 5; rep++) {
      CHK(hipEventRecord(a, s));
      for (int k = 0; k < K; k++) hipLaunchKernelGGL(noop, G, B, 0, s, st, out);
      CHK(hipEventRecord(b, s)); CHK(hipStreamSynchronize(s));
      float ms; CHK(hipEventElapsedTime(&ms, a, b)); if (ms < beste) beste = ms;
    }
    printf("no-op launches, %3d workgroups of %3d threads, %4d in a row: replayed graph %.3f us each, one by one %.3f us each (best of 5)\n", shapes[q][0], shapes[q][1], K, 1e3 * best / K, 1e3 * beste / K);
    CHK(hipGraphExecDestroy(ge)); CHK(hipGraphDestroy(g));
  }
  return 0;
}
