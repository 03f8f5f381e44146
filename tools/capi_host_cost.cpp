// Host cost of two entry points that return before any launch (no GPU needed): ns per call, best of 7 runs of 10^6 calls.
//   c++ -O2 -o capi_host_cost tools/capi_host_cost.cpp -ldl && ./capi_host_cost path/to/libmmfs_msda.so
// (profiles/op_host_layer.md: the argument checks of csrc/msda_capi.hip must not have become an allocation)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <dlfcn.h>

typedef int64_t (*workspace_fn)(int, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, unsigned);
typedef int (*forward_fn)(int, const void *, const int64_t *, const int64_t *, const void *, const void *, void *,
                          int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, void *);

template <typename F> static double best_ns(F &&call)
{
    const int n = 1000000;
    double best = 1e30;
    for (int run = 0; run < 7; ++run) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < n; ++i) call(i);
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n;
        if (ns < best) best = ns;
    }
    return best;
}

int main(int argc, char **argv)
{
    void *lib = argc > 1 ? dlopen(argv[1], RTLD_NOW) : nullptr;
    if (!lib) { fprintf(stderr, "usage: %s libmmfs_msda.so (%s)\n", argv[0], dlerror()); return 2; }
    const auto workspace = (workspace_fn)dlsym(lib, "mmfs_msda_backward_workspace_bytes");
    const auto forward = (forward_fn)dlsym(lib, "mmfs_msda_forward");
    volatile int64_t sink = 0;
    // the north star, bf16, MMFS_BWD_CANONICAL_LEVELS
    const double a = best_ns([&](int) { sink = sink + workspace(2, 8, 5440, 8, 128, 4, 4096, 4, 1u); });
    // an empty batch: dims checked, MMFS_OK before any pointer is looked at
    const double b = best_ns([&](int) { sink = sink + forward(2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 5440, 8, 128, 4, 4096, 4, nullptr); });
    printf("workspace_bytes %.1f ns   forward(empty) %.1f ns\n", a, b);
    return 0;
}
