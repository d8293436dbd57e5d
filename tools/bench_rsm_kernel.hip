// bench_rsm_kernel.hip - multinomial_counts_kernel (csrc/bm_rsm.hip) against softmax_multinomial_kernel (csrc/bm_kernels.h), the
// only other kernel of the library that turns a row of logits into counts, each alone on the same logits.  Built and run by
// tools/bench_rsm.py:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I boltzmann_machines_amd/csrc -I include \
//         tools/bench_rsm_kernel.hip -o tools/bench_rsm_kernel
//   tools/bench_rsm_kernel V J M reps        -> one JSON line
// J rows of N(0, 3^2) logits, restored from a copy in front of every launch (both kernels work in place); a launch is timed by
// one HIP event pair of its own; `reps` launches per leg behind five warm ones, the legs alternating.  Legs: the old kernel with
// its one draw count M; the new kernel with every length = M; the new kernel with lengths mixed over [20, 2 M - 20] (mean M).
#include "../boltzmann_machines_amd/csrc/bm_rsm.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace bm;

#define OK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s V J M reps\n", argv[0]); return 2; }
    const int V = atoi(argv[1]), J = atoi(argv[2]), M = atoi(argv[3]), reps = atoi(argv[4]);
    if (V < 2 || V > 8192 || J < 1 || M < 20 || reps < 1) { fprintf(stderr, "2 <= V <= 8192 (the old kernel's limit), J >= 1, M >= 20, reps >= 1\n"); return 2; }
    std::mt19937 gen(12345);
    std::normal_distribution<float> nd(0.f, 3.f);
    std::vector<float> hl((size_t)J * V), eq(J, (float)M), mixed(J);
    for (auto &x : hl) x = nd(gen);
    for (int j = 0; j < J; ++j) mixed[j] = (float)(20 + (int)(((long long)j * 7919) % (2 * M - 39)));      // [20, 2 M - 20], mean ~ M
    float *L0, *L, *S, *Deq, *Dmix;
    const size_t bytes = (size_t)J * V * sizeof(float);
    OK(hipMalloc(&L0, bytes)); OK(hipMalloc(&L, bytes)); OK(hipMalloc(&S, bytes));
    OK(hipMalloc(&Deq, J * sizeof(float))); OK(hipMalloc(&Dmix, J * sizeof(float)));
    OK(hipMemcpy(L0, hl.data(), bytes, hipMemcpyHostToDevice));
    OK(hipMemcpy(Deq, eq.data(), J * sizeof(float), hipMemcpyHostToDevice));
    OK(hipMemcpy(Dmix, mixed.data(), J * sizeof(float), hipMemcpyHostToDevice));
    hipStream_t st;
    OK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    OK(hipEventCreate(&e0)); OK(hipEventCreate(&e1));
    const PhiloxKey key{1u, 2u, 3u, 0u};
    const int max_len = 2 * M;
    auto leg = [&](int which) {
        if (which == 0) {
            SmArgs m;
            memset(&m, 0, sizeof(m));
            m.L = L; m.ld = V; m.I = V; m.J = J; m.M = M; m.sample = 1; m.states = S; m.key = key; m.row0 = 0;
            hipLaunchKernelGGL(softmax_multinomial_kernel, dim3(J), dim3(64), 2 * (size_t)V * sizeof(float), st, m);
        } else {
            McArgs a;
            memset(&a, 0, sizeof(a));
            a.L = L; a.ld = V; a.states = S; a.ld_states = V; a.lengths = which == 1 ? Deq : Dmix; a.V = V; a.J = J; a.sample = 1;
            a.max_length = max_len; a.key = key; a.row0 = 0;
            (void)launch_multinomial_counts(a, st);
        }
    };
    std::vector<float> us[3];
    for (int r = -5; r < reps; ++r)
        for (int which = 0; which < 3; ++which) {
            OK(hipMemcpyAsync(L, L0, bytes, hipMemcpyDeviceToDevice, st));
            OK(hipEventRecord(e0, st));
            leg(which);
            OK(hipEventRecord(e1, st));
            OK(hipEventSynchronize(e1));
            OK(hipGetLastError());
            float ms = 0.f;
            OK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) us[which].push_back(1e3f * ms);
        }
    auto med = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    auto mn = [](const std::vector<float> &v) { return *std::min_element(v.begin(), v.end()); };
    printf("{\"V\": %d, \"J\": %d, \"M\": %d, \"reps\": %d, \"old_us\": [%.2f, %.2f], \"new_equal_us\": [%.2f, %.2f], \"new_mixed_us\": [%.2f, %.2f]}\n",
           V, J, M, reps, med(us[0]), mn(us[0]), med(us[1]), mn(us[1]), med(us[2]), mn(us[2]));
    return 0;
}
