// launch_floor.hip -- what a chain of dependent launches on one stream costs per launch on this device,
// whatever the kernels do: the floor under a round of the greedy cover / thinning (three launches).
// A chain of 300 empty kernels between two events, for the grids the round's sweeps use at 140^3
// (one workgroup; 670 x 512, the count sweeps; 1680 x 256, the xy minimum; 1340 x 256, the select sweeps)
// and for the old one-thread-per-voxel select grid (10 719 x 256).  Best and median of nine chains.
// build: hipcc -O3 --offload-arch=gfx950 tools/ubench/launch_floor.hip -o tools/ubench/launch_floor
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
__global__ void empty_kernel(int *p) { if (p && threadIdx.x == 0x7FFFFFFF) *p = 0; }
int main() {
    if (hipSetDevice(0) != hipSuccess) { printf("no device\n"); return 1; }
    hipStream_t s;
    if (hipStreamCreate(&s) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int grids[][2] = {{1, 64}, {670, 512}, {1680, 256}, {1340, 256}, {10719, 256}};
    const int chain = 300, reps = 9;
    for (const auto &g : grids) {
        float us[reps];
        for (int r = -1; r < reps; ++r) {                      // (r = -1: warm-up)
            (void)hipEventRecord(e0, s);
            for (int i = 0; i < chain; ++i) empty_kernel<<<dim3(g[0]), dim3(g[1]), 0, s>>>(nullptr);
            (void)hipEventRecord(e1, s);
            if (hipStreamSynchronize(s) != hipSuccess) { printf("launch failed\n"); return 1; }
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (r >= 0) us[r] = ms * 1000.0f / chain;
        }
        std::sort(us, us + reps);
        printf("{\"grid\": %d, \"block\": %d, \"chain\": %d, \"us_per_launch_best\": %.2f, \"us_per_launch_median\": %.2f}\n",
               g[0], g[1], chain, us[0], us[reps / 2]);
    }
    return 0;
}
