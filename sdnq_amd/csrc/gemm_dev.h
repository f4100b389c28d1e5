// What the GEMM units share -- gemm.hip and the three that began as copies of parts of it, gemm_aq.hip, gemm_ks.hip and gemm_w4.hip: the
// block -> tile map, the hosted weight prefetch, the small templates around them, the launchers' host helpers and the prototypes of the
// functions that cross these units.  One definition each: a fix to the tile order lands in every kernel.
//
// The device functions take VALUES, never a kernel's parameter struct: the kernels are compiled with kernarg preload and decide themselves,
// with SDNQ_KERNARGS_NOW, when an argument is fetched.  What goes in wave-uniform comes out wave-uniform: tile coordinates feed buffer
// descriptors, and one of them in a VGPR puts a readfirstlane "waterfall" loop around every LDS-DMA (tools/check_spills.py --waterfalls).
// Folding a site into a helper must leave the kernel's instructions as they were: tools/compare_kernels.py shows it.  Where it did not --
// the staged 16-bit output stores of the three 8-wave kernels, gemm.hip's plain-division walk -- the site keeps its own spelling.
#pragma once
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "sdnq_dev.h"

// ---- functions that cross the GEMM units (internal to the library, C++ linkage, not part of the C ABI of include/sdnq_hip.h): declared
// here and nowhere else.  The defining unit includes this too, so the compiler sees declaration and definition side by side.
// gemm.hip: the pending weight-prefetch hint handed to another unit's launcher
int sdnq_internal_take_prefetch(int64_t room, int threads, const uint8_t* pf_ptr[4], int pf_lines[4]);
// gemm.hip: the float MFMA GEMM behind sdnq_hip_linear_float (linear_float.hip) and sdnq_hip_linear_float_multi
int sdnq_float_gemm(const void* x, const void* w, const void* bias, int dtype, void* out, int64_t m, int64_t n, int64_t k,
                    int64_t ldx, hipStream_t s, void* const* outs = nullptr, int n_outs = 0, int64_t seg_n = 0, int64_t ldc = 0);
// gemm.hip: the same kernels with a float32 store and no bias (sdnq_hip_linear_float_f32out: the cols of a transposed convolution)
int sdnq_float_gemm_f32out(const void* x, const void* w, int dtype, float* out, int64_t m, int64_t n, int64_t k, int64_t ldx, int64_t ldc,
                           hipStream_t s);
// gemm_ks.hip: the 64 x 80 tile with an in-workgroup K split (8 waves, partial sums reduced through LDS) -- tile id 28 of gemm.hip
bool sdnq_internal_ks_eligible(int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb);
bool sdnq_internal_ks_preferred(int64_t m, int64_t n, int64_t k);
int sdnq_internal_scaled_mm_ks(const void* a, const void* b, const float* sa, const float* sb, const void* bias, int bias_dtype, void* out,
                               int out_dtype, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc, hipStream_t s);
// hooks of the tests and labs, bound by their mangled names (tests/aq_internal.py, tools/aq_lab.py, tools/ks_lab.py)
void sdnq_internal_ks_trace(unsigned long long* device_buf);
void sdnq_internal_aq_trace(unsigned long long* device_buf);
void sdnq_internal_aq_geometry(int geometry);
void sdnq_internal_aq_direct(int form);
void sdnq_internal_aq_plan(int mm_dtype, long long m, long long n, long long k, int cus, long long* out);
void sdnq_internal_aq_plan_grouped(long long m, long long n_member, long long n_members, long long k, int cus, long long* out);

// ---- device side ---------------------------------------------------------------------------------------------------------------------
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// f(integral_constant<0>), ..., f(integral_constant<N-1>): a compile-time unrolled count
template <int N, int I = 0, typename F> __device__ __forceinline__ void static_for_up(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for_up<N, I + 1>(f);
    }
}

// lab: phase stamp `slot` (0..7) of this workgroup into `trace` (1024 x 8 uint64 of shader clock, or null)
#define SDNQ_PHASE_STAMP(trace, slot)                                                                                                      \
    do {                                                                                                                                   \
        if ((trace) != nullptr && threadIdx.x == 0 && blockIdx.x < 1024) (trace)[blockIdx.x * 8 + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)

// L2-aware tile order, step 1.  Block b runs on XCD b % 8 (private 4 MiB L2 each): give every XCD a CONTIGUOUS range of the sequence of
// `nwg` tiles.  Returns the position of block `bid` in that sequence.
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8, j = bid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

// Step 2: the sequence itself is grouped -- `group_m` row blocks are walked together, m fastest, so the ~32 workgroups resident on one
// XCD at a time cover a near-square patch of tiles and share both their activation strips and their weight slabs in that L2 (a 1 x 32 row
// of tiles would re-fetch every weight slab from MALL / HBM for each strip: measured 51 % of wave cycles parked on vmcnt / barrier at
// 16384 x 8192 x 4096).  For the one-launch Linear, whose K loop streams the weight operand alone, the ~20 tiles an XCD holds then share
// few weight blocks and read more distinct activation rows, all of them requested at once up front; n fastest -- every column tile of
// two row blocks per XCD -- ran its K loop at 850 cycles per stage against 730 for the two-operand loop of gemm.hip: half of its weight
// pieces missed L2.  Plain division: gemm.hip walks the same order with magic multipliers (and keeps a plain fallback of its own beside them).
__device__ __forceinline__ void grouped_tile(int pos, int tiles_m, int tiles_n, int group_m, int& tile_m, int& tile_n) {
    const int per_group = group_m * tiles_n;
    const int gid = pos / per_group, first_m = gid * group_m;
    const int gsz = (tiles_m - first_m) < group_m ? (tiles_m - first_m) : group_m;
    const int in_g = pos - gid * per_group;
    tile_n = in_g / gsz;
    tile_m = first_m + in_g - tile_n * gsz;
}

// The body of a prefetch workgroup.  A launcher appends such workgroups when the launch leaves workgroup slots free
// (sdnq_hip_prefetch_hint, launch_one in gemm.hip): they run beside the tiles on CUs that would idle and read one dword of every 128-byte
// line of the NEXT layers' weights, nothing kept -- the lines are in the Infinity Cache when their own GEMM asks for them.  Thread `tid` of
// workgroup `wg`, of `nt` threads, of `nwgs` such workgroups; `p` is the kernel's parameter struct (pf_ptr[4], pf_lines[4]).  A macro, not
// a function: as an inlined function the same loop changed the register allocation of every kernel that hosts it.
#define SDNQ_PREFETCH_LINES(tid, wg, nt, nwgs, p)                                                                           \
    do {                                                                                                                    \
        const int t = (wg) * (nt) + (tid), stride = (nwgs) * (nt);                                                          \
        _Pragma("nounroll") for (int r = 0; r < 4; ++r) {                                                                   \
            const uint8_t* base = (p).pf_ptr[r];                                                                            \
            const int lines = (p).pf_lines[r];                                                                              \
            for (int i = t; i < lines; i += stride) {                                                                       \
                int v;                                                                                                      \
                asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(base + (int64_t)i * 128) : "memory");          \
            }                                                                                                               \
        }                                                                                                                   \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                    \
    } while (0)

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// an integer from the environment; the callers cache it (`static const`) where they read it
inline int64_t env_int(const char* name, int64_t dflt) {
    const char* e = getenv(name);
    return e ? atoll(e) : dflt;
}

// compute units of the CURRENT device (a process may drive different parts / partitions); 256 when it cannot be asked
inline int cu_count() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int v = cus[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cus[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

// Allow kernel `kern` `bytes` of dynamic LDS, once per device: the attribute belongs to the function ON ONE DEVICE, so a process that
// drives several GPUs sets it once per device, not once.  `attr_devices` is the caller's `static std::atomic<uint64_t>` of this kernel
// instantiation, one bit per device.  False when the runtime refuses.
inline bool allow_dynamic_lds(const void* kern, int bytes, std::atomic<uint64_t>& attr_devices) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(attr_devices.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
        attr_devices.fetch_or(bit, std::memory_order_release);
    }
    return true;
}
