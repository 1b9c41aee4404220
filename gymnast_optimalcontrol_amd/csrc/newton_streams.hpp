// Newton solver kernels: kernel-argument constants, stream load/store wrappers and index helpers.
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

constexpr int BLK = 64;           // one wavefront per workgroup for the per-lane recursions
constexpr int STAT_BLOCKS = 256;  // first stage of the deterministic statistics reduction
constexpr int STAT_THREADS = 256;
constexpr int NSTAT = 8;
constexpr int CKI = GYM_CKPT_INTERVAL;   // state checkpoint interval (GYM_FLAG_X_CKPT)

// Cost weights as the kernels take them: the reference's diagonal Q, R, Q_T plus the Gauss-Newton
// blocks' constants (Q_t = 2Q, R_t = 2R, G00 = 2 R0 and its inverse), formed once on the host so that
// they are kernel arguments (SGPRs) rather than per-lane VGPRs.  2x is exact and 1/G00 correctly rounded
// on both sides, so the values are those the device would compute.
struct KW {
    double Q[4], R[2], QT[4];
    double twoQ[4], G00, twoR1, iG00;
};
static_assert(sizeof(Dyn) == 12 * sizeof(double) && sizeof(KW) == 17 * sizeof(double), "kernarg layout");
// KW of one gym_weights, on the host (every entry point's kernel argument) and on the device (a row of a per-lane
// table, newton_weights.hpp) by these same single-rounded operations: 2x is exact and the reciprocal is the IEEE
// division on both sides, so a row that equals the batch's weights gives the batch's KW bit for bit.
__host__ __device__ __forceinline__ KW kw(const gym_weights& w) {
    KW k;
    for (int i = 0; i < 4; ++i) { k.Q[i] = w.Q[i]; k.QT[i] = w.QT[i]; k.twoQ[i] = 2.0 * w.Q[i]; }
    k.R[0] = w.R[0]; k.R[1] = w.R[1];
    k.G00 = 2.0 * w.R[0]; k.twoR1 = 2.0 * w.R[1]; k.iG00 = 1.0 / k.G00;
    return k;
}

// The solver kernels take (Dyn m, KW w, ...) as their FIRST two parameters, i.e. at byte offsets 0 and 96 of
// the kernel argument segment.  Inside the stage loops the sweep re-reads them from there every stage with
// scalar loads (the pointer is made opaque per call so the loads are not hoisted): they are then short-
// lived SGPRs instead of 36 loop-invariant dwords that overflow the SGPR file, whose spills to VGPR lanes
// cost one v_readlane (a VALU slot) per dword per stage.
typedef const __attribute__((address_space(4))) double* kptr_t;
struct KArgs {
    Dyn m;
    KW w;
};
__device__ __forceinline__ KArgs kernarg_consts() {
    kptr_t p = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    KArgs a;
    a.m.b = p[0]; a.m.d = p[1]; a.m.a2b = p[2]; a.m.bb = p[3]; a.m.dad = p[4]; a.m.g1 = p[5]; a.m.g2 = p[6];
    a.m.f1 = p[7]; a.m.f2 = p[8]; a.m.h = p[9]; a.m.h2 = p[10]; a.m.h6 = p[11];
    for (int i = 0; i < 4; ++i) { a.w.Q[i] = p[12 + i]; a.w.QT[i] = p[18 + i]; a.w.twoQ[i] = p[22 + i]; }
    a.w.R[0] = p[16]; a.w.R[1] = p[17];
    a.w.G00 = p[26]; a.w.twoR1 = p[27]; a.w.iG00 = p[28];
    return a;
}
// The kernels whose one parameter is a by-value argument struct T (PhaseArgs, RunArgs, TailArgs) re-read its fields
// from the kernel-argument segment at each use, through a generic pointer made opaque per call (inferred back to
// scalar loads): no pointer or control value is held in SGPRs across the stage loops.
template <class T>
__device__ __forceinline__ const T* kernarg() {
    const __attribute__((address_space(4))) T* p =
        (const __attribute__((address_space(4))) T*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const T*)p;
}

typedef double d2v __attribute__((ext_vector_type(2)));

// streamed (read-once / write-once per pass) accesses: non-temporal
__device__ __forceinline__ double2 ld_nt(const double2* p) {
    const d2v v = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ double ld_nt(const double* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_nt(double2* p, double a, double b) {
    d2v v = {a, b};
    __builtin_nontemporal_store(v, reinterpret_cast<d2v*>(p));
}
__device__ __forceinline__ void st_nt(double* p, double a) { __builtin_nontemporal_store(a, p); }

// Completes the prefetch loads of the first stage before a software-pipelined stage loop is entered
// (an empty asm that reads the registers forces the wait here, in the preheader).  Without it the loop
// header merges the preheader's pending loads with the back edge's pending stores, and the compiler
// then waits for every store of the previous stage at the top of each iteration, i.e. one full HBM
// write round trip per stage.
// Solver streams through buffer instructions: the stage row's base address lives in a wave-uniform
// buffer resource (SGPRs, rebased per stage by scalar adds), the lane's byte offset in one 32-bit VGPR
// and the row-within-stage offset in an SGPR.  Compared with 64-bit per-lane pointers this frees ~14
// VGPRs and the per-stage 64-bit address arithmetic.  Offsets stay below 2^31 (Bp <= GYM_MAX_BP).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
constexpr int kNT = 2;  // gfx950 cache-policy bits: nt (streamed once; other policies measured, profiles/r05/policy)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const char* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), (short)0, 0x7fffffff, 0x00020000);
}
template <int CP = kNT>   // CP: cache policy (kNT for the read-once solver streams, 0 for re-read ones)
__device__ __forceinline__ double2 bld2(__amdgpu_buffer_rsrc_t r, uint32_t vo, uint32_t so) {
    return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, CP));
}
template <int CP = kNT>
__device__ __forceinline__ double bld1(__amdgpu_buffer_rsrc_t r, uint32_t vo, uint32_t so) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, CP));
}
template <int CP = kNT>
__device__ __forceinline__ void bst2(__amdgpu_buffer_rsrc_t r, uint32_t vo, uint32_t so, double a, double b) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, make_double2(a, b)), r, vo, so, CP);
}
template <int CP = kNT>
__device__ __forceinline__ void bst1(__amdgpu_buffer_rsrc_t r, uint32_t vo, uint32_t so, double a) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, a), r, vo, so, CP);
}

__device__ __forceinline__ void pin(double v) { asm volatile("" : : "v"(v)); }

// Progress-banded wave priority: every solver stream loop starts at priority 3 and steps down one level
// per quarter of its stages.  Without it the SIMD's oldest-first issue arbitration runs the oldest of its
// (at most 4) resident waves far ahead of the youngest (measured: the ranks finish at 0.88 / 1.39 / 1.95
// / 2.49 ms of a 2.5 ms launch), so the launch ends with one wave per SIMD and few loads in flight.  With
// the bands the lagging waves win arbitration, all finish together, and the launch is 6% shorter.
// The stage index is wave-uniform: these are scalar compares and s_setprio, no VALU.
// KIND: 0 = sweep, 1 = trial, 2 = no banding (the caller sets the priority).  (Measured alternatives: sweep
// banded above the trial, 1.3% slower; trial above the sweep, 9.6% slower.)
constexpr int PRIO_NONE = 2;
template <int KIND>
__device__ __forceinline__ void prio_start() {
    if (KIND != PRIO_NONE) __builtin_amdgcn_s_setprio(3);
}
template <int KIND>
__device__ __forceinline__ void prio_band(int done, int T) {
    if (KIND == PRIO_NONE) return;
    asm volatile("" : "+s"(T));   // thresholds recomputed per stage (3 SALU) rather than held: no spills
    if (done >= ((3 * T) >> 2)) __builtin_amdgcn_s_setprio(0);
    else if (done >= (T >> 1)) __builtin_amdgcn_s_setprio(1);
    else if (done >= (T >> 2)) __builtin_amdgcn_s_setprio(2);
}
__device__ __forceinline__ void pin(double2 v) { asm volatile("" : : "v"(v.x), "v"(v.y)); }

// element index of (t, row p of P, lane) in a time-major plane stream (W = 1 doubles): (L, P, Bp)
__device__ __forceinline__ int64_t pix(int t, int p, int P, int64_t l, int64_t Bp) { return ((int64_t)t * P + p) * Bp + l; }
// Per-lane references (GYM_FLAG_REF_LANE, every schedule): x_ref (Bp, N, 4), u_ref (Bp, T, 2), lane-major.
// RL kernels offset the reference pointers by the lane once; everything downstream reads stage t at +4t / +2t as
// with the shared reference (then by vector instead of scalar loads: the same values, the same bits).
// Call sites spell out the (xr, 4N) / (ur, 2(N-1)) pair in argument position: one helper returning both rows moves
// the address arithmetic ahead of the other operands' loads and changes the schedule of 28 kernels
// (tools/kernel_isa_diff.py).
template <bool RL>
__device__ __forceinline__ const double* lane_ref(const double* r, int64_t l, int64_t per_lane) {
    return RL ? r + l * per_lane : r;
}
// element index of (t, row p of P, lane) in a wave-blocked pair stream (W = 2, double2): (L, Bp/64, P, 64), i.e.
// the P rows of one wavefront's 64 lanes at one stage form one contiguous P KiB block (one DRAM burst sequence
// instead of P 1-KiB pieces Bp*16 bytes apart).  The stage stride is P*Bp elements, as for planes.
__device__ __forceinline__ int64_t wix(int64_t t, int p, int P, int64_t l, int64_t Bp) {
    return t * P * Bp + (l & ~(int64_t)(BLK - 1)) * P + p * BLK + (l & (BLK - 1));
}
// the same as a byte offset within one stage (buffer-resource addressing), and the row-to-row step
__device__ __forceinline__ uint32_t wbo(int64_t l, int P) {
    return (uint32_t)(((l & ~(int64_t)(BLK - 1)) * P + (l & (BLK - 1))) * 16);
}
constexpr uint32_t WROW = BLK * 16;
