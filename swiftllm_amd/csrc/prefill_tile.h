// prefill_tile.h — what the three prefill attention kernels share (gfx950): prefill_attn_kernel and
// prefill_attn_dma_kernel (prefill_attn.hip), prefill_attn_paged_kernel (prefill_attn_paged.hip). One workgroup is 4 waves,
// a wave owns 32 q rows and walks the keys in 64-key tiles; what is here is everything that does not know how a tile
// reached LDS: the decode of the 1-D grid, the direct Q^T fragment load, the tile body (S^T = K.Q^T, mask, online softmax,
// O^T += V^T.P^T) and the whole-row epilogue. A kernel brings its staging and two fragment readers. One body means the
// kernels agree to the bit by construction.
#pragma once

#include "attn_mfma.h"

namespace swl {

constexpr int kBQ = 128; // q rows per workgroup (LDS-DMA kernel: (4 / hpw) * 32)
constexpr int kBK = 64;  // keys per LDS tile (paged kernel: four pool blocks)

// ---- XCD-aware decode of the 1-D grid ---------------------------------------------------------------------------------
// Workgroup id -> XCD id & 7 round-robin (the hardware's dispatch order), so unit = (sequence, kv-head) `xcd + 8 n` keeps
// all its q blocks and all its q-heads on one XCD and their shared K/V in that XCD's L2; inside a unit the q blocks are
// taken longest (latest rows) first. A workgroup holds `hpw` q-heads of the kv-head (LDS-DMA kernel; the others pass a
// literal 1 and the head-group arithmetic folds away); num_q_blocks counts blocks of the workgroup's rows.
struct PrefillGrid {
    bool valid;     // false: a padding unit past num_seqs * KVH — the workgroup leaves
    int seq, kvh;
    int hgroup;     // first q-head of the workgroup = kvh * G + hgroup * hpw
    int qb;         // q block
    static __device__ __forceinline__ PrefillGrid decode(int id, int num_seqs, int H, int KVH, int num_q_blocks, int hpw) {
        const int hgroups = H / KVH / hpw;
        const int per_unit = hgroups * num_q_blocks;
        const int xcd = id & 7;
        const int j = id >> 3;
        const int unit = xcd + 8 * (j / per_unit);
        const int inner = j % per_unit;
        return {unit < num_seqs * KVH, unit / KVH, unit % KVH, inner % hgroups, num_q_blocks - 1 - inner / hgroups};
    }
};

// Host side of the same: workgroups of the grid (units padded to the 8 XCDs); false when they do not fit 31 bits.
static inline bool prefill_grid_blocks(int num_seqs, int KVH, int hgroups, int num_q_blocks, dim3 *grid) {
    const int64_t units = static_cast<int64_t>(num_seqs) * KVH;
    const int64_t nblocks = (units + 7) / 8 * 8 * hgroups * num_q_blocks;
    if (nblocks > 0x7fffffffLL) return false;
    *grid = dim3(static_cast<unsigned>(nblocks));
    return true;
}

// ---- Q^T B-fragments, loaded directly: lane holds Q[qrow][kk*16 + hf*8 .. +8]; rows past the sequence are zeros ----------
template <typename T, int D>
__device__ __forceinline__ void prefill_load_q(vec8_t<T> (&qf)[D / 16], const T *qg, int start, int head,
                                               int64_t q_tok_stride, int qrow, int len, int hf) {
    const bool ok = qrow < len;
    const T *qp = qg + (static_cast<int64_t>(start) + (ok ? qrow : 0)) * q_tok_stride + static_cast<int64_t>(head) * D + hf * 8;
#pragma unroll
    for (int kk = 0; kk < D / 16; ++kk) {
        vec8_t<T> t = load8(qp + kk * 16);
        if (!ok) t = vec8_t<T>{};
        qf[kk] = t;
    }
}

// ---- one 64-key tile of one wave --------------------------------------------------------------------------------------
// qf: Q^T fragments; ot / m_run / l_run: the wave's O^T accumulators and this lane's row state (lane l owns q row l % 32,
// the keys of a tile are split with lane ^ 32). c = scale * log2(e). The tile is on the wave's diagonal when `diagonal`;
// a key is then masked when its index in the tile exceeds dmask = (the row's last visible key) - key0 - 4 hf.
// kfrag(t, kk): the vec8_t<T> A fragment of keys 32 t .. 32 t + 31, k-step kk. vfrag(t, ks, dt, half): the short4_t of one
// transpose read of V rows 32 t + 16 ks + 8 half .., columns 32 dt ... PRIO brackets the MFMA blocks with s_setprio
// (favour the wave that is feeding the matrix pipe: a gain with the barrier-coupled register staging, a 1.4-1.7 % loss
// with two free-running LDS-DMA workgroups per CU — profiles/r06b_prefill_attn_setprio_ab.jsonl).
// The body issues NO global memory access: the LDS-DMA kernel's counted waits rely on it.
template <typename T, int D, bool PRIO, typename KFrag, typename VFrag>
__device__ __forceinline__ void prefill_tile(const vec8_t<T> (&qf)[D / 16], float16_t (&ot)[D / 32], float &m_run,
                                             float &l_run, float c, int dmask, bool diagonal, KFrag kfrag, VFrag vfrag) {
    constexpr int KSTEPS = D / 16, DT = D / 32;
    // ---- S^T = K . Q^T  (two 32-key sub-tiles) ------------------------------------------------
    float16_t st[2];
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        st[t] = float16_t{};
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) {
            const vec8_t<T> kf = kfrag(t, kk);
            st[t] = mfma32(kf, qf[kk], st[t]);
        }
    }
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
    // S^T is read by VALU next, behind the diagonal-tile branch (swl_common.h)
    mfma_results_tie(st[0]);
    mfma_results_ready<8>(st[1]);
    // causal mask on the diagonal tiles (keys past the sequence's end are > every valid q row as well)
    if (diagonal) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // key > row with key = key0 + 32 t + (r & 3) + 8 (r >> 2) + 4 hf: a compile-time constant against ONE
                // per-lane value (one compare + one select per element; r01-r06a rebuilt the key first: three)
                if ((r & 3) + 8 * (r >> 2) + t * 32 > dmask) st[t][r] = kNegBig;
            }
    }
    // ---- online softmax: this lane owns q row l32, keys split with lane^32 ---------------------
    float mx = st[0][0];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[t][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // lazy running maximum (r06b): a row moves its maximum only when the tile raised it by more than kLazyMax (base-2
    // exponent units), so p stays <= 2^kLazyMax instead of <= 1 — 16-bit floats round p to the same RELATIVE precision at
    // either scale, l and O accumulate in fp32 — and alpha is exactly 1 for that row: the 64-multiply rescale of O below
    // then fires on the first tile or two of a row block instead of on most tiles (any of a wave's 32 rows setting a
    // record). Decided per ROW, so a row's arithmetic still depends on its own scores only (the causality test holds
    // bit for bit).
    const float m_cand = fmaxf(m_run, mx * c);
    const float m_new = m_cand - m_run > kLazyMax ? m_cand : m_run;
    const float alpha = fast_exp2(m_run - m_new);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pv = fast_exp2(fmaf(st[t][r], c, -m_new));
            st[t][r] = pv;
            psum += pv;
        }
    l_run = fmaf(l_run, alpha, psum);
    // rescale O only when some row of this wave actually raised its max (alpha == 1 otherwise: after the first tiles of
    // a sequence that is the common case) — a wave-uniform branch that removes 16*DT multiplies per lane per tile
    if (!__all(alpha == 1.0f)) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
    }

    // ---- O^T += V^T . P^T ------------------------------------------------------------------------
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
    // k-step (t, ks): this lane's 8 k-slots are keys t*32 + 16*ks + 4*hf + {0..3} and + 8 + {0..3}
    // == accumulator registers 8*ks .. 8*ks+7 of st[t] — identical order on both operands.
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            vec8_t<T> pb;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) pb[jj] = to_t<T>(st[t][8 * ks + jj]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const short4_t lo = vfrag(t, ks, dt, 0);
                const short4_t hi = vfrag(t, ks, dt, 1);
                typedef short short8_t __attribute__((ext_vector_type(8)));
                const short8_t both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                ot[dt] = mfma32(__builtin_bit_cast(vec8_t<T>, both), pb, ot[dt]);
            }
        }
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
}

// ---- epilogue: O[q0w + row][d] = O^T[d][row] / l (* v_scale) ---------------------------------------------------------
// Written as WHOLE ROWS: a lane holds 4 consecutive d of ONE row per register quad, so a direct store instruction touches
// 32 rows a token pitch apart with 2 x 8 bytes each — 16 such instructions per lane, the store-issue-bound tail the in-box
// guide prices at ~4 us per workgroup (T21). The wave's 32 x D tile goes through LDS instead and comes back row-major,
// 16 bytes per lane, 16 lanes = one 256-byte row: 8 full-line stores per lane at D = 128 (r04; r01-r03 stored the pieces).
// `ow` is this wave's 32 rows of pitch D + 8 in the dead K/V tiles: the CALLER puts the barrier after the last tile and
// asserts that four such tiles fit its LDS. The tile is wave-private: LDS operations of one wave complete in order, no
// barrier between the writes and the reads. obase = the o row of token 0 of the sequence at this wave's head.
// SCALED (FP8 pools) multiplies by v_scale in fp32 before the one rounding. It is a template flag and not a factor of 1:
// without it float16 fuses product and rounding into one v_fma_mixlo/hi_f16, the exact product rounded once; the FP8 form
// rounds the product to fp32 first: 1 ulp apart on rare ties.
// l32 = lane & 31 and hf = lane >> 5 are the KERNEL's values, handed in: derived again here they are new instructions
// to the scheduler, and the FP8 D = 128 kernel then reads its K fragments one per MFMA instead of in pairs — in the
// LOOP, +0.9 % on chunked 16k prompts (profiles/prefill_tile_shared_speed_vs_parent.jsonl, first session).
template <typename T, int D, bool SCALED>
__device__ __forceinline__ void prefill_store_rows(float16_t (&ot)[D / 32], float l_run, float v_scale, T *ow, T *obase,
                                                   int64_t o_tok_stride, int q0w, int len, int lane, int l32, int hf) {
    constexpr int DT = D / 32, ORS = D + 8, CPR = D / 8;
    constexpr int RPI = 64 / CPR;                    // rows per store instruction
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) mfma_results_tie(ot[dt]);
    mfma_results_ready<8>(ot[DT - 1]);
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            typename Vec4<T>::type ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x = ot[dt][4 * r4 + e] * inv;
                if constexpr (SCALED) x *= v_scale;
                ov[e] = to_t<T>(x);
            }
            *reinterpret_cast<typename Vec4<T>::type *>(ow + l32 * ORS + dt * 32 + 8 * r4 + 4 * hf) = ov;
        }
#pragma unroll
    for (int i = 0; i < 32 / RPI; ++i) {
        const int row = i * RPI + lane / CPR, ch = lane % CPR;
        const vec8_t<T> v = *reinterpret_cast<const vec8_t<T> *>(ow + row * ORS + ch * 8);
        if (q0w + row < len) store8(obase + static_cast<int64_t>(q0w + row) * o_tok_stride + ch * 8, v);
    }
}

} // namespace swl
