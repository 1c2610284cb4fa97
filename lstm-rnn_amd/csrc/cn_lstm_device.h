// Device helpers shared by the recurrent LSTM kernels (cn_lstm.hip, cn_lstm_s2.hip, cn_lstm_cluster.hip): the reference's
// activation functions and LSTM cell (forward and backward), the 16x16 MFMA steps, the split-bf16 operands, the gradient
// sums and the LDS-only workgroup barrier.
#pragma once

#include <hip/hip_runtime.h>

namespace cn {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(8))) unsigned u32x8;
typedef __attribute__((ext_vector_type(16))) __bf16 bf16x16;

#define LOG2E 1.4426950408889634f

// Logistic::fn (Logistic.cuh:33-44).  The reference clamps to exactly 0 / 1 beyond |x| >= 88.72; both
// forms below reach the same limits without a branch (exp overflows to +inf -> 1/inf = 0; exp underflows
// -> 1/(1+0) = 1).  F32: libm-grade expf and IEEE division; bf16 mode: v_exp_f32 / v_rcp_f32.
template <bool F32>
__device__ __forceinline__ float logistic(float x)
{
    if constexpr (F32) return 1.0f / (1.0f + expf(-x));
    else return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * x));
}
// Tanh::fn = Maxmin1::fn(2x) = 2*Logistic::fn(2x) - 1 (Tanh.cuh:33-36, Maxmin1.cuh:33-36)
template <bool F32>
__device__ __forceinline__ float tanh_ref(float x)
{
    if constexpr (F32) return 2.0f * (1.0f / (1.0f + expf(-2.0f * x))) - 1.0f;
    else return __builtin_fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.0f * LOG2E * x)), -1.0f);
}
__device__ __forceinline__ float clip1(float e) { return fminf(fmaxf(e, -1.0f), 1.0f); }   // limitedError.cuh:31-34

// one 64-byte K chunk of a 16x16 tile product: 32 bf16 (one MFMA) or 16 fp32 (four MFMAs; the K order
// inside the chunk is permuted identically for A and B)
template <bool F32>
__device__ __forceinline__ void mma16(f32x4 &acc, const u32x4 &a, const u32x4 &b)
{
    if constexpr (F32) {
        // (bit_cast the whole vector: a bit_cast of a single ext_vector element picks element 0)
        const f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[i], acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                      __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
}

// Row pitch of an MFMA A-operand tile in LDS (16 rows read as ds_read_b128 at row*pitch + 16*(lane>>4)).
// ds_read_b128 is served in groups of 16 lanes ({0-3,12-15,20-27}, ...) that mix rows of two k-quarters,
// so it is conflict-free exactly when pitch/16 = 2 (mod 4); a pitch of row + 16 B is a 2-way conflict on
// every read (SQ_LDS_BANK_CONFLICT = 4 cycles per read, measured).
__host__ __device__ constexpr int lds_pitch(int row_bytes)
{
    return row_bytes + 16 * ((2 - (row_bytes / 16) % 4 + 4) % 4);
}

// ---- split-bf16 ("bf16x3") operands -----------------------------------------------------------------------------
// x = hi + lo + r with hi = bf16(x), lo = bf16(x - hi), |r| <= 2^-17 |x| (two 8-bit significands, round to nearest):
// a product a*b ~ ah*bh + al*bh + ah*bl drops al*bl (2^-18) and the two r terms (2^-17 each): ~2^-16 relative per term
// with fp32 accumulation, against 2^-9 for plain bf16 operands and 2^-24 for fp32.
__device__ __forceinline__ void split_bf16(float x, __bf16 &hi, __bf16 &lo)
{
    hi = (__bf16)x;
    lo = (__bf16)(x - (float)hi);
}
// eight consecutive fp32 (two 16-byte vectors) -> one MFMA fragment of 8 bf16 hi and one of 8 bf16 lo
__device__ __forceinline__ void split8(const f32x4 &x0, const f32x4 &x1, u32x4 &hi, u32x4 &lo)
{
    bf16x8 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        __bf16 a, b;
        split_bf16(x0[i], a, b); h[i] = a; l[i] = b;
        split_bf16(x1[i], a, b); h[4 + i] = a; l[4 + i] = b;
    }
    hi = __builtin_bit_cast(u32x4, h); lo = __builtin_bit_cast(u32x4, l);
}
// three bf16 MFMAs of one 32-element K chunk of a 16x16 tile product (small terms first)
__device__ __forceinline__ void mma16_x3(f32x4 &acc, const u32x4 &ah, const u32x4 &al, const u32x4 &bh, const u32x4 &bl)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
}

// ---- 2:4 "row pair" products (v_smfmac_f32_16x16x64_bf16) -----------------------------------------------------------
// The 16-row A tile of a recurrent step holds 4*RPL sequences, so with RPL <= 2 at least half of its rows are padding and
// the dense MFMA spends its cycles on them.  The sparse MFMA multiplies a 16 x 64 A whose rows keep 2 of every 4 K
// positions (8 stored values + eight 2-bit positions per lane) with a dense 64 x 16 B in the cycles of the dense
// 16x16x32 (measured, tools/probe/smfmac_probe.hip: 17-18 cycles per instruction on 1, 2 or 8 accumulators).  Two tile
// rows share one sequence: the even row keeps positions {0,1} of every group of four, the odd row {2,3}; both are fully
// dense in their stored values, so nothing is pruned -- the product is exact, the K = 64 chunk costs one instruction
// instead of two, and the sequence's sum is D[even row] + D[odd row], both in the lane's own registers.
// Operand pairing (measured with unit impulses, same probe): A lane (row = lane & 15, j = lane >> 4), stored slot s with
// position field v meets B lane (col = lane & 15, j' = 2*(j & 1) + (s >> 2)) slot 8*(j >> 1) + 4*((s >> 1) & 1) + v; the
// position fields of a lane are bits [15:0] of the index register (ABID = 0).  With B lane j' slot i holding k' = 16*j' + i
// (16 consecutive K values per lane, two 16-byte loads), value k' of a sequence belongs in tile row parity (k' >> 1) & 1 at
// stored position sp_pos(k') of its 32-value row chunk; a reader lane takes its 8 slots with one ds_read_b128 at
// row*pitch + 64*chunk + 16*j, the same expression as for the dense tile.
__device__ __forceinline__ constexpr int sp_parity(int k) { return (k >> 1) & 1; }
__device__ __forceinline__ constexpr int sp_pos(int k)
{
    return 16 * ((k >> 3) & 1) + 8 * ((k >> 5) & 1) + 4 * ((k >> 4) & 1) + 2 * ((k >> 2) & 1) + (k & 1);
}
// index register of a reader lane: even tile rows keep positions {0,1}, odd rows {2,3} of every group
__device__ __forceinline__ int sp_index(int row) { return (row & 1) ? (int)0xEEEEEEEEu : 0x44444444; }
__device__ __forceinline__ u32x8 sp_join(const u32x4 &lo, const u32x4 &hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ void smma16(f32x4 &acc, const u32x4 &a, const u32x8 &b, int idx)
{
    acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x16, b), acc, idx, 0, 0);
}
// split operands (P_X3): small terms first, as mma16_x3
__device__ __forceinline__ void smma16_x3(f32x4 &acc, const u32x4 &ah, const u32x4 &al, const u32x8 &bh, const u32x8 &bl, int idx)
{
    smma16(acc, al, bh, idx);
    smma16(acc, ah, bl, idx);
    smma16(acc, ah, bh, idx);
}
// 16 consecutive K values of one B column as a sparse-product fragment: bf16 in memory, or fp32 split into hi and lo
__device__ __forceinline__ u32x8 sp_load_bf16(const void *p) { return sp_join(*(const u32x4 *)p, *((const u32x4 *)p + 1)); }
__device__ __forceinline__ void sp_load_split(const float *p, u32x8 &hi, u32x8 &lo)
{
    u32x4 h0, l0, h1, l1;
    split8(*(const f32x4 *)p, *(const f32x4 *)(p + 4), h0, l0);
    split8(*(const f32x4 *)(p + 8), *(const f32x4 *)(p + 12), h1, l1);
    hi = sp_join(h0, h1); lo = sp_join(l0, l1);
}

// Keeps every lane of an MFMA accumulator tuple allocated until `after` (a value computed from the tuple's results) exists.
// Lanes whose rows are never read are dead to the register allocator, which may hand them to another value while the MFMA
// that will still write them is in flight.  For ordinary instructions the hazard recognizer then inserts the wait states; the
// staged-operand copies of these kernels are inline asm, which it does not look into: observed once (an experimental build,
// T = 1 path): `v_smfmac v[140:143]` followed by the asm copy `v_mov_b32 v142, ...`, overwritten when the MFMA retired.
// The pin is part of a kernel's instruction stream (the register allocator reacts to where it sits): it stays at the call
// site, at its point of the data flow.
#define KEEP_TUPLE(tuple, after) asm volatile("" :: "v"(tuple), "v"(after))

// element `elem` of an array of T at a wave-uniform base: the byte offset stays a 32-bit VGPR (saddr form)
template <typename T> __device__ __forceinline__ T &at32(const void *base, unsigned elem)
{
    return *(T *)((char *)base + elem * (unsigned)sizeof(T));
}

// ---- the LSTM cell ----------------------------------------------------------------------------------------------------
// What differs between kernels (where the gate sums come from, the KEEP_TUPLE pins, the stamps, the stores) stays at the call
// site.  The arithmetic has two forms that are NOT interchangeable:
//   contracted (EXPLICIT = false): plain C++ expressions, a * b + c left to the compiler's contraction -- lstm_fwd_kernel
//     here; the cluster kernels and the contracted backward kernels (lstm_bwd_kernel, lstm_bwd_cluster_kernel,
//     lstm_bwd_cluster_psum_kernel) still state this form in place: moved behind a call they compile to other register
//     counts, spills and packed / scalar multiplies (tools/isa_same.py), so they wait for a spelling that does not;
//   explicit (EXPLICIT = true / lstm_cell_bwd_explicit): the fused operations written out -- the compiled twins of the
//     hand-written and generated loops (lstm_fwd_s2_kernel, lstm_fwd_s2w_kernel, lstm_bwd_s2_kernel, lstm_bwd_s2c_kernel),
//     which tests hold bit-equal to those loops: their rounding must not depend on the optimiser.
// Forward, ComputeBlockOutputFn (LstmLayer.cu:87-136): s = the four gate sums n, i, f, o (bias and recurrent part inside), cp
// the previous cell state.  co / yo are the cell state and the output with dummy slots zeroed (:78-85, in both directions here);
// the activations and th of a dummy slot are never read back.
struct CellOut { float ni, ig, fg, og, th, co, yo; };
template <bool ACC, bool EXPLICIT>
__device__ __forceinline__ CellOut lstm_cell_fwd(const float (&s)[4], float cp, float pi, float pf, float po, bool dummy)
{
    CellOut c;
    c.ni = tanh_ref<ACC>(s[0]);
    c.ig = logistic<ACC>(s[1] + cp * pi);
    c.fg = logistic<ACC>(s[2] + cp * pf);
    float cs;
    if constexpr (EXPLICIT) cs = __builtin_fmaf(c.ni, c.ig, cp * c.fg);
    else cs = c.ni * c.ig + cp * c.fg;
    c.og = logistic<ACC>(s[3] + cs * po);
    c.th = tanh_ref<ACC>(cs);
    const float y = c.th * c.og;
    c.yo = dummy ? 0.f : y;
    c.co = dummy ? 0.f : cs;
    return c;
}

// what a backward step hands to the next one (the step of t+1 in time order): forget gate, cell state error, input and
// forget gate deltas; all zero at firstCall
struct CellCarry { float fg, ec, dig, dfg; };

// Backward, ComputeBlockErrorsFn (LstmLayer.cu:236-285), as an explicit operation sequence: e = outputErrors + the recurrent
// product, a = the activations n, i, f, o, th = tanh(cell state), cp the previous cell state (0 at lastCall); out come the
// deltas, clipped when stored (:281-285; the cell state error is not, and ec uses the unclipped dog, :262-263), and the carry
// is updated in place.  No contraction is left to the compiler: the hand-written and generated backward loops issue exactly
// these operations and are held bit-equal.  Everything that does not depend on e is formed first -- in
// the hand-written loops one step early, in the shadow of the LDS hand-off --, and the dummy-slot rule enters as a factor
// m = 0 / 1, so that behind the product only
//   dog = [m og (1 - og) th] e,   ec = e [m (og (1 - th^2) + po og (1 - og) th)] + m (fg' ec' + pi dig' + pf dfg')
//   dni = [m ig (1 - ni^2)] ec,   dfg = [m fg (1 - fg) cp] ec,   dig = [m ig (1 - ig) ni] ec      (' = carried from t+1)
// remain: one multiply or fma each, then the clips.
__device__ __forceinline__ void lstm_cell_bwd_explicit(float e, const f32x4 &a, float cp, float th, float pi, float pf, float po,
                                                       CellCarry &c, bool dummy, float &dni, float &dig, float &dfg, float &dog)
{
    const float ni = a[0], ig = a[1], fg = a[2], og = a[3];
    float ec;
    {
#pragma clang fp contract(off)
        const float m = dummy ? 0.f : 1.f;
        const float t2p = __builtin_fmaf(-og, og, og) * th;
        const float vp = og * __builtin_fmaf(-th, th, 1.0f);
        const float w = __builtin_fmaf(po, t2p, vp);
        const float d2p = ig * __builtin_fmaf(-ni, ni, 1.0f);
        const float d3p = __builtin_fmaf(-fg, fg, fg) * cp;
        const float d4p = __builtin_fmaf(-ig, ig, ig) * ni;
        float car = c.fg * c.ec;
        car = __builtin_fmaf(pi, c.dig, car);
        car = __builtin_fmaf(pf, c.dfg, car);
        dog = (t2p * m) * e;
        ec = __builtin_fmaf(e, w * m, car * m);
        dni = (d2p * m) * ec; dfg = (d3p * m) * ec; dig = (d4p * m) * ec;
        c.fg = fg * m;
    }
    dni = clip1(dni); dig = clip1(dig); dfg = clip1(dfg); dog = clip1(dog);
    c.ec = ec; c.dig = dig; c.dfg = dfg;
}

// The bias / peephole sums a backward workgroup has formed over its time steps and sequences for unit `unit` of direction d
// (v[0..3]: gate deltas n, i, f, o; v[4..6]: peephole terms i, f, o) leave for the gradient: one atomic per (gate, unit) and
// workgroup, or -- deterministic mode -- one plain store into the workgroup's slot of p.gpart (LstmRec, cn_internal.h).
template <typename REC>
__device__ __forceinline__ void lstm_grad_sums_out(const REC &p, int HP, int d, int unit, const float (&v)[7])
{
    if (p.gpart) {
        float *slot = p.gpart + (size_t)blockIdx.x * (size_t)(7 * p.dirs * HP);
#pragma unroll
        for (int g = 0; g < 4; ++g) slot[(d * HP + unit) * 4 + g] = p.bias * v[g];
#pragma unroll
        for (int g = 0; g < 3; ++g) slot[4 * p.dirs * HP + (d * 3 + g) * HP + unit] = v[4 + g];
        return;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) atomicAdd(&p.dbias[(d * HP + unit) * 4 + g], p.bias * v[g]);
#pragma unroll
    for (int g = 0; g < 3; ++g) atomicAdd(&p.dpeep[(d * 3 + g) * HP + unit], v[4 + g]);
}

// workgroup barrier that orders LDS traffic only: global prefetch loads and the activation stores
// stay in flight across it (a __syncthreads() would drain vmcnt every step)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace cn
