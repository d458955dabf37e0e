// ===========================================================================
// ops_instantiate.inc -- included by ops_<dtype>.hip with
//   IP_T (storage type), IP_G (coordinate type), IP_R (math type),
//   IP_ACC (scatter accumulation type), IP_SFX (symbol suffix), IP_FULL (0/1:
//   also build pushgrad/hess), IP_LOWP (0/1: 16-bit storage), IP_PART (1 gather,
//   2 scatter, 3 fused backward: one translation unit each, built in parallel).
// Defines the typed launchers the C-ABI layer (abi.hip) dispatches to.
// ===========================================================================
#include "ops_generic.hpp"
#include "launch.hpp"
#include "route.hpp"

namespace ip {

#define IP_NAME2(a, b) a##b
#define IP_NAME(a, b) IP_NAME2(a, b)

// ---- part 1: gather operators ------------------------------------------------
#if IP_PART == 1
int IP_NAME(launch_pull_, IP_SFX)(const KParams &p, const void *vol, const void *grid, void *val, int B, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        hipLaunchKernelGGL((pull_generic<IP_T, IP_G, IP_R, D, K, I>), sample_grid(p, B), dim3(BLOCK), 0, st,
                           p, (const IP_T *)vol, (const IP_G *)grid, (IP_T *)val, B, TileList{});
    });
}

int IP_NAME(launch_grad_, IP_SFX)(const KParams &p, const void *vol, const void *grid, void *val, int B, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        hipLaunchKernelGGL((grad_generic<IP_T, IP_G, IP_R, D, K, I>), sample_grid(p, B), dim3(BLOCK), 0, st,
                           p, (const IP_T *)vol, (const IP_G *)grid, (IP_T *)val, B, TileList{});
    });
}

#if IP_FULL
int IP_NAME(launch_hess_, IP_SFX)(const KParams &p, const void *vol, const void *grid, void *val, int B, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        hipLaunchKernelGGL((hess_generic<IP_T, IP_G, IP_R, D, K, I>), sample_grid(p, B), dim3(BLOCK), 0, st,
                           p, (const IP_T *)vol, (const IP_G *)grid, (IP_T *)val, B);
    });
}

#endif
#if IP_DEFER
// the samples of the tiles that an LDS-tiled kernel handed back (TileList): persistent blocks over the descriptors
static inline dim3 deferred_grid(const TileList &tl) { return dim3((unsigned)(tl.nwork < 8192 ? tl.nwork : 8192), 1u, 1u); }

int IP_NAME(launch_pull_deferred_, IP_SFX)(const KParams &p, const void *vol, const void *grid, void *val, const TileList &tl, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        hipLaunchKernelGGL((pull_generic<IP_T, IP_G, IP_R, D, K, I, true>), deferred_grid(tl), dim3(BLOCK), 0, st,
                           p, (const IP_T *)vol, (const IP_G *)grid, (IP_T *)val, 0, tl);
    });
}

int IP_NAME(launch_grad_deferred_, IP_SFX)(const KParams &p, const void *vol, const void *grid, void *val, const TileList &tl, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        hipLaunchKernelGGL((grad_generic<IP_T, IP_G, IP_R, D, K, I, true>), deferred_grid(tl), dim3(BLOCK), 0, st,
                           p, (const IP_T *)vol, (const IP_G *)grid, (IP_T *)val, 0, tl);
    });
}
#endif
#endif

// ---- part 2: scatter operators -----------------------------------------------
#if IP_PART == 2
int IP_NAME(launch_push_, IP_SFX)(const KParams &p, const void *val, const void *grid, void *acc, int B, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        if (val)
            hipLaunchKernelGGL((push_generic<IP_T, IP_G, IP_R, IP_ACC, D, K, I, false>), sample_grid(p, B), dim3(BLOCK), 0, st,
                               p, (const IP_T *)val, (const IP_G *)grid, (IP_ACC *)acc, B, TileList{});
        else
            hipLaunchKernelGGL((push_generic<IP_T, IP_G, IP_R, IP_ACC, D, K, I, true>), sample_grid(p, B), dim3(BLOCK), 0, st,
                               p, (const IP_T *)nullptr, (const IP_G *)grid, (IP_ACC *)acc, B, TileList{});
    });
}

#if IP_FULL
int IP_NAME(launch_pushgrad_, IP_SFX)(const KParams &p, const void *val, const void *grid, void *acc, int B, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        hipLaunchKernelGGL((pushgrad_generic<IP_T, IP_G, IP_R, IP_ACC, D, K, I>), sample_grid(p, B), dim3(BLOCK), 0, st,
                           p, (const IP_T *)val, (const IP_G *)grid, (IP_ACC *)acc, B);
    });
}

#endif
int IP_NAME(launch_narrow_, IP_SFX)(const void *src, void *dst, int64_t n, hipStream_t st)
{
#if IP_LOWP
    int64_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL((narrow_kernel<IP_T>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, (const float *)src, (IP_T *)dst, n);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
#else
    (void)src; (void)dst; (void)n; (void)st;
    return -4;
#endif
}

#if IP_DEFER
static inline dim3 deferred_grid(const TileList &tl) { return dim3((unsigned)(tl.nwork < 8192 ? tl.nwork : 8192), 1u, 1u); }

// val == NULL: count
int IP_NAME(launch_push_deferred_, IP_SFX)(const KParams &p, const void *val, const void *grid, void *acc, const TileList &tl, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        if (val)
            hipLaunchKernelGGL((push_generic<IP_T, IP_G, IP_R, IP_ACC, D, K, I, false, true>), deferred_grid(tl), dim3(BLOCK), 0, st,
                               p, (const IP_T *)val, (const IP_G *)grid, (IP_ACC *)acc, 0, tl);
        else
            hipLaunchKernelGGL((push_generic<IP_T, IP_G, IP_R, IP_ACC, D, K, I, true, true>), deferred_grid(tl), dim3(BLOCK), 0, st,
                               p, (const IP_T *)nullptr, (const IP_G *)grid, (IP_ACC *)acc, 0, tl);
    });
}
#endif

#endif

// ---- part 3: fused backward operators ----------------------------------------
#if IP_PART == 3
int IP_NAME(launch_pullbwd_, IP_SFX)(const KParams &p, const void *gout, const void *vol, const void *grid, void *gvol,
                                     void *ggrid, int B, int64_t gsb, int64_t gsc, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        hipLaunchKernelGGL((pullbwd_generic<IP_T, IP_G, IP_R, IP_ACC, D, K, I>), sample_grid(p, B), dim3(BLOCK), 0, st,
                           p, (const IP_T *)gout, (const IP_T *)vol, (const IP_G *)grid, (IP_ACC *)gvol, (IP_G *)ggrid, B, gsb, gsc, TileList{});
    });
}

int IP_NAME(launch_pushbwd_, IP_SFX)(const KParams &p, const void *gvol_out, const void *val, const void *grid, void *gval,
                                     void *ggrid, int B, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        if (val)
            hipLaunchKernelGGL((pushbwd_generic<IP_T, IP_G, IP_R, D, K, I, false>), sample_grid(p, B), dim3(BLOCK), 0, st,
                               p, (const IP_T *)gvol_out, (const IP_T *)val, (const IP_G *)grid, (IP_T *)gval, (IP_G *)ggrid, B, TileList{});
        else
            hipLaunchKernelGGL((pushbwd_generic<IP_T, IP_G, IP_R, D, K, I, true>), sample_grid(p, B), dim3(BLOCK), 0, st,
                               p, (const IP_T *)gvol_out, (const IP_T *)nullptr, (const IP_G *)grid, (IP_T *)gval, (IP_G *)ggrid, B, TileList{});
    });
}

#if IP_DEFER
static inline dim3 deferred_grid(const TileList &tl) { return dim3((unsigned)(tl.nwork < 8192 ? tl.nwork : 8192), 1u, 1u); }

int IP_NAME(launch_pullbwd_deferred_, IP_SFX)(const KParams &p, const void *gout, const void *vol, const void *grid, void *gvol,
                                              void *ggrid, int64_t gsb, int64_t gsc, const TileList &tl, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        hipLaunchKernelGGL((pullbwd_generic<IP_T, IP_G, IP_R, IP_ACC, D, K, I, true>), deferred_grid(tl), dim3(BLOCK), 0, st,
                           p, (const IP_T *)gout, (const IP_T *)vol, (const IP_G *)grid, (IP_ACC *)gvol, (IP_G *)ggrid, 0, gsb, gsc, tl);
    });
}

// val == NULL: backward of count
int IP_NAME(launch_pushbwd_deferred_, IP_SFX)(const KParams &p, const void *gvol_out, const void *val, const void *grid, void *gval,
                                              void *ggrid, const TileList &tl, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        if (val)
            hipLaunchKernelGGL((pushbwd_generic<IP_T, IP_G, IP_R, D, K, I, false, true>), deferred_grid(tl), dim3(BLOCK), 0, st,
                               p, (const IP_T *)gvol_out, (const IP_T *)val, (const IP_G *)grid, (IP_T *)gval, (IP_G *)ggrid, 0, tl);
        else
            hipLaunchKernelGGL((pushbwd_generic<IP_T, IP_G, IP_R, D, K, I, true, true>), deferred_grid(tl), dim3(BLOCK), 0, st,
                               p, (const IP_T *)gvol_out, (const IP_T *)nullptr, (const IP_G *)grid, (IP_T *)gval, (IP_G *)ggrid, 0, tl);
    });
}
#endif

#endif

} // namespace ip
