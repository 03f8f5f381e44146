// Host cost of four entry points that return before any launch (no GPU needed): ns per call, best of 7 runs of 10^6 calls.
//   c++ -O2 -o capi_host_cost tools/capi_host_cost.cpp -ldl && ./capi_host_cost path/to/libmmfs_msda.so
// (profiles/op_host_layer.md, profiles/module_host_layer.md: the argument checks must not have become an allocation)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <dlfcn.h>

typedef int64_t (*workspace_fn)(int, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, unsigned);
typedef int (*forward_fn)(int, const void *, const int64_t *, const int64_t *, const void *, const void *, void *,
                          int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, void *);
typedef int (*rmsnorm_fn)(int, const void *, const void *, void *, float *, int64_t, int64_t, float, void *);
typedef int (*train_bwd_fn)(int, const void *, const void *, const void *, const void *, const void *, const float *,
                            const int64_t *, const float *, const float *, int64_t, void *, void *, void *, float *, int64_t,
                            int64_t, int64_t, int64_t, void *);

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
    // the module: an empty batch; the longest pointer list with its last pointer off by 4 (fake addresses, 1 MiB apart:
    // MMFS_E_ALIGN comes back before anything is launched)
    const auto rmsnorm = (rmsnorm_fn)dlsym(lib, "mmfs_rmsnorm_forward");
    const auto train_bwd = (train_bwd_fn)dlsym(lib, "mmfs_llama_attn_train_backward");
    auto at = [](uintptr_t i) { return (char *)(i << 20); };
    auto empty_norm = [&] { return rmsnorm(2, nullptr, nullptr, nullptr, nullptr, 0, 4096, 1e-6f, nullptr); };
    auto misaligned_bwd = [&] {
        return train_bwd(2, at(1), at(2), at(3), at(4), at(5), (const float *)at(6), (const int64_t *)at(7), (const float *)at(8),
                         (const float *)(at(9) + 4), 4096, at(10), at(11), at(12), (float *)at(13), 2, 512, 8, 128, nullptr);
    };
    if (empty_norm() != 0 || misaligned_bwd() != -4) { fprintf(stderr, "a module call is not the one it was written as\n"); return 1; }
    const double c = best_ns([&](int) { sink = sink + empty_norm(); });
    const double e = best_ns([&](int) { sink = sink + misaligned_bwd(); });
    printf("workspace_bytes %.1f ns   forward(empty) %.1f ns   rmsnorm_forward(empty) %.1f ns   train_backward(misaligned) %.1f ns\n",
           a, b, c, e);
    return 0;
}
