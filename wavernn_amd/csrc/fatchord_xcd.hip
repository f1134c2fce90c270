// fatchord_xcd.hip — XCD-resident persistent kernel for MoL rows (rnn 512, fc 512): the sample
// loop of models/fatchord_version.py:201-241 for ONE row on the 32 CUs of ONE XCD, up to eight
// rows (one per XCD) per launch.
//
// Why one XCD: every hand-off of the loop is an all-gather among the workgroups that hold the
// weights.  Kept inside one XCD, a granule can be published with a PLAIN store — the line stays
// in that XCD's L2, where the consumers' sc1 polls find it — instead of an sc1 store that goes
// to the Infinity Fabric: tools/xcdbench.hip measures 0.23 µs one-way (0.41 sc1 same-XCD, 0.59
// cross-XCD), tools/xcdhop.hip 0.50 µs per 32 → 32 all-gather hop (1.16 spread over 8 XCDs).
// The 11.4 MB of loop weights fit the XCD's 32 CUs as 96 KB of W_hh1 per CU in LDS and the rest
// (W_ih2, fc1, fc2 rows, fc3 columns, W_hh2) in the VGPRs of 8 waves (two per SIMD).
//
// Workgroup c of an XCD owns GRU units 16c..16c+15 (both GRUs) and fc rows 16c..16c+15.  Every
// critical role has its own waves (fatchord_xcd.h): GRU2 on waves 0, 5, 6, 7 (one per SIMD, four
// units each), fc1 on waves 1, 2, fc2 on waves 3, 4, the sampler on wave 0 — so each hop's
// pollers publish nothing in that hop's window and are already polling when its rows land.
// Per step t (x = x_{t-1}):
//   GRU1 for ALL units, one per thread, from the gathered terms S (rank-1 in x: no hop) → B2
//   waves 0, 5..7: W_ih2·h1 for the wave's 12 gate rows (VGPR weights, h1 from LDS) → GRU2 gates
//        (r, z of an engine's two units in its lanes 0..3, the n rows reduced under their sigmoids,
//        h' in lanes 0 / 2) → publish y = x_I + h1 + h2                              [hop Y]
//   waves 1, 2 (polling Y from B2 on): fc1 rows (8 per wave) → relu → publish f1  [hop F1]
//   waves 3, 4: fc2 rows → relu → fc3 partial logits of the workgroup's 16 f2 rows; wave 4 hands
//        its partials to wave 3 (LDS) → publish 30 partials                        [hop F2]
//   wave 0 gathers all 32 × 30 partials, sums + b3, samples (MoL, utils/distribution.py:87-123,
//   redundantly and bit-identically in every workgroup) → x_t → step-end barrier.
// Off the critical path: W_hh1·h1 (LDS weights, waves 0, 3, 4, 5, 7) → the GRU1 terms of step
// t+1 → publish (hop S, double-buffered); h2 published by the GRU2 waves after "y gathered",
// gathered by wave 6 → W_hh2·h2 (VGPR rows of waves 1..7 + LDS rows) for the next GRU2; S
// gathered by waves 1, 2, 5 and fc2 wave 4, a quarter each; the conditioning terms and noise of
// step t+2 into the LDS ring (wave 7; one-shot launches find the sampler's noise terms prepared in the
// terms record, the windowed ones form them there).
//
// Membership: each workgroup reads its XCC id from the hardware register and takes an index
// from a per-XCD arrival counter, so correctness never depends on the dispatcher's placement
// (a missing member shows up as a bounded-wait timeout, never as a hang).  Arithmetic is fp32
// with the sums re-associated (tolerance-checked against the oracle like the other kernels).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fatchord_loop.h"
#include "fatchord_xcd.h"
#include "wrnn_device.h"
#include "xcd_device.h"

namespace wrnn {

// diagnostics (tools/ab_libs.sh): skip an off-critical exchange (wrong results, timing only)
#ifndef WRNN_XCD_SKIP_SG
#define WRNN_XCD_SKIP_SG 0
#endif
#ifndef WRNN_XCD_SKIP_H2
#define WRNN_XCD_SKIP_H2 0
#endif
// diagnostics: 1 = skip ALL the off-critical recurrent work (W_hh1·h1 → the GRU1 terms S and
// their exchange, the h2 exchange, W_hh2·h2): the critical path alone, timing only — the ceiling
// of moving that work off this XCD (DESIGN.md §9.1's two-XCD-per-row idea)
#ifndef WRNN_XCD_SKIP_RECUR
#define WRNN_XCD_SKIP_RECUR 0
#endif
#ifndef WRNN_XCD_PRIO
#define WRNN_XCD_PRIO 0         // s_setprio of wave 0 (the poller / sampler)
#endif

// the wave that gathers the fourth quarter of the next step's GRU1 terms: 4 (an fc2 wave, idle
// after its fc3 hand-off) — wave 6 gathered it after h2, and its W_hh2·h2 then ended with the
// sampler (both at the step-end barrier); 6: as before, 3: the other fc2 wave (A/B)
#ifndef WRNN_XCD_SQ3_WAVE
#define WRNN_XCD_SQ3_WAVE 4
#endif
// 1: the sampler wave's first F2 poll waits for fc2 wave 4's LDS hand-off (hop F2 cannot be complete before
// the workgroup's own line is on its way): from its GRU1-term publish on, wave 0 polled F2 for 0.9 µs with 8
// loads a round, on the SIMD of fc2 wave 4 and through the L2 that carries hops F1 and F2; 0: as before (A/B)
#ifndef WRNN_XCD_F2_GATE
#define WRNN_XCD_F2_GATE 1
#endif
#ifndef WRNN_XCD_STAMP_W13
#define WRNN_XCD_STAMP_W13 5    // stamped builds: the wave whose W_hh2·h2 end is stamp 13 (6: the h2 gatherer)
#endif
#define XSTAMPW(kk, w)                                                                                        \
    do {                                                                                                      \
        if (kDbg && a.dbg && wave == (w) && lane == 0 && t - t0 < a.dbg_steps &&                            \
            (!WRNN_XCD_BAR_STAMPS || ((kk) != 3 && ((kk) < 9 || (kk) > 14))))                                 \
            a.dbg[((size_t)mem * a.dbg_steps + (t - t0)) * kStamps + (kk)] = (unsigned)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define XSTAMP(kk) XSTAMPW(kk, 0)
// diagnostics (WRNN_XCD_BAR_STAMPS): waves 1..6 → stamps 9..14, wave 7 → stamp 3, at the step-end barrier
#define XSTAMP_BAR()                                                                                          \
    do {                                                                                                      \
        if (WRNN_XCD_BAR_STAMPS && kDbg && a.dbg && wave > 0 && lane == 0 && t - t0 < a.dbg_steps)          \
            a.dbg[((size_t)mem * a.dbg_steps + (t - t0)) * kStamps + (wave == 7 ? 3 : 8 + wave)] =          \
                (unsigned)__builtin_amdgcn_s_memrealtime();                                                   \
    } while (0)

// The set-up of one piece of work inside fatchord_xcd_kernel (the launch's one window; kLst: every piece
// of the lane's queue — a macro, because the list form needs the text twice and a lambda shared with the
// other instantiations changes their code): ring slots t0..t0+2, the carried state (the loads consumed by
// an empty asm use so the wait lands before the loop: left pending, their first use inside it is an
// s_waitcnt vmcnt(0) in EVERY step, draining all the wave's in-flight publishes and loads there), the
// GRU1 terms of step 0 (GH1 = 0) published and gathered, x_{t-1} and the GRU1 terms of the first step.
// Returns from the kernel when the launch was aborted.
#define XCD_PIECE_BEGIN()                                                                                     \
    do {                                                                                                      \
        {                                                                                                     \
            for (int t = t0; t < t0 + 3; ++t) {                                                               \
                if (t <= t_terms)                                                                             \
                    for (int i = tid; i < kXTerms; i += kXThreads) RING(t)[i] = TERMS(t)[i];                  \
                if constexpr (kWin)                                                                           \
                    if (wave == 1 && lane < 11 && t < nz_hor) NZ(t)[lane] = noise_term(t);                    \
            }                                                                                                 \
        }                                                                                                     \
        resume = t0 > 0;                                                                                      \
        if constexpr (kGrp) st = rw.state + (size_t)c * kXStateW;                                             \
        else st = a.state + ((size_t)k * kXcdWgs + c) * kXStateW;                                             \
        h1v = resume ? st[tid] : 0.0f;                                                                        \
        h2own = resume ? st[512 + 2048 + 48 + ui] : 0.0f;                                                     \
        asm volatile("" : "+v"(h1v), "+v"(h2own));                                                            \
        if (resume) {                                                                                         \
            for (int i = tid; i < 4 * R; i += kXThreads) sg[i] = st[512 + i];                                 \
            if (tid < 48) gh2s[tid] = st[512 + 2048 + tid];                                                   \
            if (tid == 0) xs[(t0 + 1) & 1] = st[512 + 2048 + 48 + 16];                                        \
        } else {                                                                                              \
            if (tid < 48) gh2s[tid] = 0.0f;                                                                   \
            if (tid == 0) xs[1] = 0.0f;                                                                       \
        }                                                                                                     \
        __syncthreads();                                                                                      \
        if (!resume) {                                                                                        \
            if (gh1w) {                                                                                       \
                const float z5[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};                                           \
                publish_terms(0, z5);                                                                         \
            }                                                                                                 \
            if (wave == 1 || wave == 2 || wave == 5 || wave == WRNN_XCD_SQ3_WAVE) {                           \
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                              \
                gather_terms(0);                                                                              \
            }                                                                                                 \
        }                                                                                                     \
        __syncthreads();                                                                                      \
        if (*abort_flag) return;                                                                              \
        x = xs[(t0 + 1) & 1];                                                                                 \
        s4 = lds4(sg + 4 * tid);                                                                              \
    } while (0)

// … and its end: the recurrent state carried to the next time chunk (every workgroup its own copy)
#define XCD_PIECE_END()                                                                                       \
    do {                                                                                                      \
        __syncthreads();                                                                                      \
        st[tid] = h1v;                                                                                        \
        for (int i = tid; i < 4 * R; i += kXThreads) st[512 + i] = sg[i];                                     \
        if (tid < 48) st[512 + 2048 + tid] = gh2s[tid];                                                       \
        if (g2w && (li & ~2) == 0) st[512 + 2048 + 48 + ui] = h2own;                                          \
        if (tid == 0) st[512 + 2048 + 48 + 16] = xs[(t_end - 1) & 1];                                         \
    } while (0)

__device__ __forceinline__ const XcdArgs &launch_args(const XcdArgs &ka) { return ka; }
__device__ __forceinline__ const XcdArgs &launch_args(const XcdGroupArgs &ka) { return ka.a; }
__device__ __forceinline__ const XcdArgs &launch_args(const XcdListArgs &ka) { return ka.a; }

// kGrp (grouped launches, fatchord_xcd.h: XcdRow): the row's window, operands and results come from
// row k of the table instead of the launch-wide fields; the steps themselves are the same code
// kLst (list launches, fatchord_xcd.h: XcdPiece; a kGrp whose row changes): XCD k walks a queue of
// pieces in device memory.  Membership and the resident weights are set up once per launch; per
// piece only the window, the operand bases, the ring and the state — and the step loop runs as it is.
//
// Tags at a piece boundary.  Every tagged word carries step + 1 of the utterance it serves, and a
// new utterance restarts at step 0, so a word left by the previous piece could pass for one of the
// next piece's steps.  Neither kind can:
//   * hand-off granules (global): an utterance has a granule region of its own, zeroed before the
//     call and kept across its rounds.  Consecutive pieces of a lane within one launch belong to
//     DIFFERENT utterances (a piece ends where its utterance or the round ends), so a step of piece
//     B polls only words that B's own steps wrote, or zero; the tags an utterance left in an
//     earlier round are those of steps before t0 (the GRU1 terms of step t0 come back from the
//     state record, not from a gather), below every tag the resumed piece waits for — a session's
//     chunks rely on the same.
//     For the same reason no barrier spans the XCD at a boundary: a workgroup already in B and one
//     still in A touch disjoint regions, and B's first hand-off waits for B's publishers as any
//     step does.  The state record is per workgroup (each reads and writes its own slice only).
//   * LDS words (misc[2..7], the f2x pairs): all waves of the workgroup pass the barrier behind
//     the piece's last step, store the state, pass a second barrier (nobody reads the old piece's
//     LDS any more), then the words are zeroed — tag 0, which no step carries — ahead of the
//     barrier that precedes the new piece's first flag wait.
// The launch runs ONE step loop over the lane's time: the piece switch is a cold block at the end
// of a piece's last step.  A piece loop around the step loop kept the lane-invariant part AND the
// per-piece sum of every per-lane address alive across the steps and spilled into the step.
template <bool kDbg, bool kWin, bool kGrp = false, bool kLst = false>
__global__ __launch_bounds__(kXThreads, 2) void fatchord_xcd_kernel(
    std::conditional_t<kLst, XcdListArgs, std::conditional_t<kGrp, XcdGroupArgs, XcdArgs>> ka) {
    static_assert(!kGrp || (kWin && !kDbg), "grouped launches are windowed and carry no stamps");
    static_assert(!kLst || kGrp, "a list launch is a grouped one whose rows come from the piece queue");
    const XcdArgs &a = launch_args(ka);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 512, TW = kXcdWgs * kXTerms;
    const XcdLds ll = xcd_lds_layout();
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, eng = lane >> 5;
    // the wave index wave-uniform (SGPR): its role branches become scalar, its offsets scalar operands
    const int wave = WRNN_XCD_UNIFORM_WAVE ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    float *whh1 = smem + ll.whh1, *whh2l = smem + ll.whh2, *f2x = smem + ll.f2x, *h1s = smem + ll.h1, *h2s = smem + ll.h2, *sg = smem + ll.sg, *w3s = smem + ll.w3;
    float *ring = smem + ll.ring, *nzr = smem + ll.nz, *gh2s = smem + ll.gh2, *cst = smem + ll.cst, *xs = smem + ll.xs;
    int *misc = reinterpret_cast<int *>(smem + ll.misc);
    int *abort_flag = misc, *h2ready = misc + 2, *ypub = misc + 3, *ygot = misc + 4, *f1got = misc + 5;

    // ---- membership: XCD k (row b0 + k) and index c within it
    if (tid == 0) {
        const int k = (int)xcc_id();
        int c = kXcdWgs;
        if constexpr (kLst) {   // a lane whose timeline has ended takes no XCD
            const bool in = k < a.nb && ka.first[k + 1] > ka.first[k];
            if (in) c = atomicAdd(&a.members[k], 1);
            misc[1] = (in && c < kXcdWgs) ? k * kXcdWgs + c : -1;
        } else if constexpr (kGrp) {   // a row without steps takes no XCD: its workgroups leave here
            const bool in = k < a.nb && ka.row[k].Lc > 0;
            if (in) c = atomicAdd(&a.members[k], 1);
            misc[1] = (in && c < kXcdWgs) ? k * kXcdWgs + c : -1;
        } else {
            if (k < a.nb) c = atomicAdd(&a.members[k], 1);
            misc[1] = (k < a.nb && c < kXcdWgs) ? k * kXcdWgs + c : -1;
        }
        misc[0] = 0;
        for (int i = 2; i < 8; ++i) misc[i] = 0;
    }
    if (tid < 64) f2x[tid] = 0.0f;   // the fc3 hand-off pairs: tag 0, which no step carries
    __syncthreads();
    const int mem = __builtin_amdgcn_readfirstlane(misc[1]);   // wave-uniform: hop addresses in SGPRs
    if (mem < 0) return;
    const int k = mem / kXcdWgs, c = mem - k * kXcdWgs;
    const int b = a.b0 + k;
    // the row's step window: the launch's, or (kGrp) its own — k is wave-uniform, the table reads scalar
    int t0, Lc, L;
    XcdRow rw{};   // kGrp: row k of the table, read once here; kLst: the piece being run
    [[maybe_unused]] int pi = 0, pend = 0;   // kLst: the lane's queue position and end
    if constexpr (kLst) {
        pi = ka.first[k];
        pend = ka.first[k + 1];
        rw = list_piece<XcdRow>(ka.pieces, pi);
        t0 = rw.t0;
        Lc = rw.Lc;
        L = rw.L;
    } else if constexpr (kGrp) {
        rw = ka.row[k];
        t0 = rw.t0;
        Lc = rw.Lc;
        L = rw.L;
    } else {
        t0 = a.t0;
        Lc = a.Lc;
        L = a.L;
    }
    int t_end = t0 + Lc;
    int t_terms = min(t_end, L - 1);
    int nz_hor;   // the step below which injected draws exist
    if constexpr (kGrp) nz_hor = rw.nz_hor;
    else nz_hor = kWin ? a.nz_hor : L;
    unsigned long long *xg;
    if constexpr (kGrp) xg = rw.xg;
    else xg = a.xg + (size_t)k * kXXcdStride;
    auto XG = [&](int hop) { return xg + (size_t)hop * kXHopStride; };
    // publishes through one wave-uniform buffer descriptor + a 32-bit granule index (the 64-bit
    // per-lane pointers of each hop stayed live across the loop and were spilled: the F2 publish
    // reloaded its address from scratch and waited vmcnt(0) on the critical path)
    __amdgpu_buffer_rsrc_t xgr = __builtin_amdgcn_make_buffer_rsrc(xg, 0, 0x7fffffff, 0x00020000);
    auto XGI = [&](int hop) { return hop * (int)kXHopStride; };
    auto RING = [&](int t) { return ring + (t & (kXRing - 1)) * kXTerms; };
    auto NZ = [&](int t) { return nzr + (t & (kXRing - 1)) * kXNoise; };
    auto TERMS = [&](int t) {
        if constexpr (kGrp) return rw.terms + (size_t)(t - t0) * (size_t)rw.terms_ld + (size_t)c * kXTerms;
        else return a.terms + ((size_t)(t - t0) * a.nb + k) * TW + (size_t)c * kXTerms;
    };
    const float *S = a.slab + (size_t)c * a.s.total;
    unsigned long long prow, seed;
    if constexpr (kGrp) {
        prow = (unsigned long long)rw.row;
        seed = rw.seed;
    } else {
        prow = (unsigned long long)(a.row0 + k);
        seed = a.seed;
    }

    // ---- register-resident weights: one role-indexed set of 28 float4 (chunks li + 32m of a row)
    //   GRU2 waves (0, 5..7; group g2): W_ih2 gate q of unit 4·g2 + 2j + e (slab pair 2·g2 + j) as
    //     three row pairs interleaved for e32part2, W[8p + 0..7]: (a_r, a_z), (b_r, b_z), (a_n, b_n)
    //     with a, b the units j = 0, 1; W[24 + m]: W_hh2 pass 7 + w (waves 5..7; wave 0: none — its
    //     F2 poll buffer is a transient of the poll, when no GRU2 operand is live)
    //   waves 1, 2 / 3, 4: W[0..15] fc1 / fc2 rows 8h + r, r = 0..7, at the granules this lane polls,
    //     as four row pairs (fc8_rows_rp); W[16 + 4p + m]: W_hh2 passes 3(w − 1) + p, p = 0..2
    f4v W[28];
    auto ldrow = [&](const float *row, int m) { return *reinterpret_cast<const f4v *>(row + 4 * (li + 32 * m)); };
    const bool fcw = wave >= kXWaveFc1 && wave < kXWaveFc2 + 2;
    const bool g2w = !fcw;
    const int g2 = g2w && wave != 0 ? wave - 4 : 0;  // GRU2 group (GRU2 waves)
    if (fcw) {
        const int hf = (wave - kXWaveFc1) & 1;
        const float *Wf = S + (wave < kXWaveFc2 ? a.s.w1 : a.s.w2) + hf * 8 * R;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const f2v ra = *reinterpret_cast<const f2v *>(Wf + 2 * p * R + 2 * (lane + 64 * kk));
                const f2v rb = *reinterpret_cast<const f2v *>(Wf + (2 * p + 1) * R + 2 * (lane + 64 * kk));
                W[4 * p + kk] = f4v{ra.x, rb.x, ra.y, rb.y};
            }
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int m = 0; m < 4; ++m) W[16 + 4 * p + m] = ldrow(S + a.s.whh2 + (2 * (3 * (wave - 1) + p) + eng) * R, m);
    } else {
        auto g2row = [&](int j, int q) { return S + a.s.wih2 + ((2 * g2 + j) * 6 + 2 * q + eng) * R; };
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const float *ra = g2row(p == 1 ? 1 : 0, p == 2 ? 2 : 0), *rb = g2row(p == 0 ? 0 : 1, p == 2 ? 2 : 1);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f4v wa = ldrow(ra, m), wb = ldrow(rb, m);
                W[8 * p + 2 * m] = f4v{wa.x, wb.x, wa.y, wb.y};
                W[8 * p + 2 * m + 1] = f4v{wa.z, wb.z, wa.w, wb.w};
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
            W[24 + m] = wave != 0 ? ldrow(S + a.s.whh2 + (2 * (7 + wave) + eng) * R, m) : f4v{0.0f, 0.0f, 0.0f, 0.0f};
    }
    auto W4 = [&](int i) -> const f4v(&)[4] { return *reinterpret_cast<const f4v(*)[4]>(&W[i]); };
    auto W4x8 = [&](int i) -> const f4v(&)[8] { return *reinterpret_cast<const f4v(*)[8]>(&W[i]); };
    auto W4x16 = [&]() -> const f4v(&)[16] { return *reinterpret_cast<const f4v(*)[16]>(&W[0]); };
    // GRU1 of unit tid: x-coefficients
    const float q1r = S[a.s.q1a + tid], q1z = S[a.s.q1a + R + tid], q1n = S[a.s.q1a + 2 * R + tid];
    // GRU2 waves: the local GRU2 unit this lane works for (lanes 0, 1 of an engine: its first unit,
    // lanes 2, 3: its second; lanes 0 / 2 form r, tanh and h', lanes 1 / 3 z; the other lanes
    // compute along, their results are not used) and the gate whose sigmoid it forms
    const int ui = 4 * g2 + (li & 2) + eng, gq = li & 1;
    // W_hh1 rows (waves 0, 3, 4, 5: ten each, wave 7: eight): gh0 + 2p + e, p = 0..4; lane li < 5
    // of an engine publishes the terms of its row gh0 + 2·li + e
    const bool gh1w = wave == 0 || wave == 3 || wave == 4 || wave == 5 || wave == 7;
    const int gh0 = wave == 0 ? 0 : wave == 7 ? 40 : 10 * (wave - 2);
    // sampler noise of step t → NZ(t): u1 → log(-log u1) (distribution.py:107), u2 → log u2 − log(1 − u2) (:119).
    // One-shot launches (!kWin) find these terms in slot XT_NZ of the step's terms record, written per
    // row-step by xcd_draws_kernel ahead of the launch, so they come into the ring with the record: a Philox
    // word and three logf per step, the same in all 32 workgroups, stood on wave 7's way to the step-end
    // barrier.  The windowed, grouped and list launches still form them here.
    [[maybe_unused]] auto noise_term = [&](int t) -> float {
        float uu;
        if constexpr (kGrp) {
            if (rw.noise) uu = rw.noise[(size_t)t * (size_t)rw.noise_ld + lane];
            else uu = philox_noise(seed, prow, (uint32_t)t, (uint32_t)lane, 1);
        } else {
            if (a.noise) uu = a.noise[((size_t)t * a.Bt + b) * 11 + lane];
            else uu = philox_noise(seed, prow, (uint32_t)t, (uint32_t)lane, 1);
        }
        return mol_noise_term(uu, lane);
    };
    // GRU1 term(s) of step t for W_hh1 row rr (u·3 + q), by lane 0 / 32 of an engine:
    //   q = 0: S_r = (GH1_r + b_hh,r) + (P1_r + b_ih,r), q = 1: S_z likewise,
    //   q = 2: Gh_n = GH1_n + b_hh,n (term 3) and Gi_n = P1_n + b_ih,n (term 2)
    auto publish_term = [&](int t, int rr, float gh) {
        const int u = rr / 3, q = rr - 3 * u;
        const float p1 = RING(t)[XT_P1 + rr], bh = cst[XC_BHH1 + rr], bi = cst[XC_BIH1 + rr];
        const int g = XGI(XH_S0 + (t & 1)) + (c * kXUnits + u) * 4;
        const uint32_t tag = (uint32_t)t + 1u;
        if (q < 2) {
            xpub_b(xgr, g + q, tag, (gh + bh) + (p1 + bi));
        } else {
            xpub_b(xgr, g + 3, tag, gh + bh);
            xpub_b(xgr, g + 2, tag, p1 + bi);
        }
    };
    // the GRU1 terms of this wave's W_hh1 rows (gh[p]: row gh0 + 2p + e), lanes li < 5
    auto publish_terms = [&](int t, const float (&gh)[5]) {
        const int rr = gh0 + 2 * li + eng;
        if (li < 5 && rr < 48) {
            const float v = li == 0 ? gh[0] : li == 1 ? gh[1] : li == 2 ? gh[2] : li == 3 ? gh[3] : gh[4];
            publish_term(t, rr, v);
        }
    };
    // W_hh1·h1 for this wave's rows (the GRU1 terms of step t + 1, published later by
    // publish_terms): all dots first, so LDS reads of later rows overlap earlier dots
    auto gh1_dots = [&](float (&gh)[5]) {
        f4v hx[4];
        e32x(h1s, li, hx);
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            f4v w4[4];
            e32x(whh1 + min(gh0 + 2 * p + eng, 47) * R, li, w4);
            gh[p] = e32dot(w4, hx);
        }
    };
    // intra-workgroup step flags in LDS (no data behind them, or the writer drained its LDS
    // stores first): the critical waves mark "y gathered" / "f1 gathered", the others wait for
    // them so that their own memory traffic stays out of the critical hops' windows
    auto set_flag = [&](int *f, uint32_t tag) {
        if (lane == 0) __hip_atomic_store(f, (int)tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto wait_flag = [&](int *f, uint32_t tag) {
        while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != (int)tag)
            __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    };
    // W_hh2·h2 → gh2s for the next GRU2 (after wave 6 has gathered h2): lanes li < np store the
    // rows rb + 2·li + e
    auto gh2_store = [&](int rb, int np, const float (&gh)[5]) {
        const int rr = rb + 2 * li + eng;
        if (li < np) gh2s[rr] = li == 0 ? gh[0] : li == 1 ? gh[1] : li == 2 ? gh[2] : li == 3 ? gh[3] : gh[4];
    };
    // W_hh2 LDS passes p0 .. p0 + np − 1 (np ≤ 2; pass P = rows 2P + e, LDS row 2P + e − kXH2RegRows)
    auto gh2_lds = [&](int p0, int np, const f4v (&hx)[4]) {
        float gh[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (p < np) {
                f4v w4[4];
                e32x(whh2l + (2 * (p0 + p) + eng - kXH2RegRows) * R, li, w4);
                gh[p] = e32dot(w4, hx);
            }
        gh2_store(2 * p0, np, gh);
    };
    // a quarter of step t's GRU1 terms (waves 1, 2, 5, WRNN_XCD_SQ3_WAVE: 512 granules each, one
    // poll round)
    auto gather_terms = [&](int t) {
        const int qq = wave == 1 ? 0 : wave == 2 ? 1 : wave == 5 ? 2 : 3;
        xgather16<4>(XG(XH_S0 + (t & 1)) + qq * 512, (uint32_t)t + 1u, a.ctl, a.timeout_ticks, t, XH_S0 + (t & 1),
                     abort_flag, lane, [&](int i, float v0, float v1) {
                         *reinterpret_cast<f2v *>(sg + qq * 512 + i) = f2v{v0, v1};
                     });
    };

    // a GRU2 wave's four granules of a hop (units 4·g2 .. 4·g2 + 3; unit 4·g2 + 2j + e lives in lane
    // 2j of engine e): lanes 0 and 2 store the pairs (lane 2j, lane 32 + 2j) as one 16-byte store
    // each, one instruction, 32 contiguous bytes.  Engine 1's value comes by one permlane32 swap
    // (of v with itself: a lane < 32 finds lane + 32's value in the second result) instead of two
    // readlanes through SGPRs
    auto pub4 = [&](int hop, float v, uint32_t tagv) {
        const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        if ((lane & ~2) == 0)
            __builtin_amdgcn_raw_buffer_store_b128(u4v{__float_as_uint(v), tagv, s[1], tagv}, xgr,
                                                   (XGI(hop) + c * kXUnits + 4 * g2 + lane) * 8, 0, 0);
    };
    // ---- prologue: W_hh1, fc3 columns, small vectors, ring slots t0..t0+2, state
    {
        const f4v *src = reinterpret_cast<const f4v *>(S + a.s.whh1);
        f4v *dst = reinterpret_cast<f4v *>(whh1);
        for (int i = tid; i < 48 * R / 4; i += kXThreads) dst[i] = src[i];
        src = reinterpret_cast<const f4v *>(S + a.s.whh2 + kXH2RegRows * R);
        dst = reinterpret_cast<f4v *>(whh2l);
        for (int i = tid; i < kXH2LdsRows * R / 4; i += kXThreads) dst[i] = src[i];
        for (int i = tid; i < kXFcRows * 32; i += kXThreads) w3s[i] = S[a.s.w3 + i];
        for (int i = tid; i < kXCst; i += kXThreads) cst[i] = S[a.s.cst + i];
    }
    // ---- per piece of work (the launch's one window; kLst: every piece of the lane's queue): ring
    // slots t0..t0+2, the carried state, the step-0 terms; afterwards the state store
    bool resume;
    float *st;
    float h1v, h2own;   // h1 of unit tid (recurrent, this thread); h2 of this lane's GRU2 unit (GRU2 waves)
    float x;            // x_{t-1}, wave-uniform
    f4v s4;             // GRU1 terms of unit tid for step t
    XCD_PIECE_BEGIN();

    if (WRNN_XCD_PRIO && wave == 0) __builtin_amdgcn_s_setprio(WRNN_XCD_PRIO);
    // kLst: ONE step loop over the lane's time in this launch — the piece switch sits in a cold
    // block at its end, so nothing of a piece's set-up lives in registers across the steps
    for (int t = t0; t < t_end; ++t) {
        const uint32_t tag = (uint32_t)t + 1u;
        const bool more = t + 1 < L;
        const float *tr = RING(t);
        XSTAMP(0);
        if (kDbg && a.dbg && wave == 0 && lane == 0 && t - t0 < a.dbg_steps)   // shader clock beside the 100 MHz one
            a.dbg[((size_t)mem * a.dbg_steps + (t - t0)) * kStamps + 15] = (unsigned)__builtin_amdgcn_s_memtime();
        // operands of the GRU2 gate math (this lane's unit ui; [0]: the gate gq whose sigmoid the
        // lane forms, [1]: the n gate): LDS reads issued before GRU1's transcendental chain (behind
        // its h1 store the compiler could not move them).  Every wave issues them (the fc waves
        // read units 0..3 and drop the values): under a role branch their waits land at the
        // branch's join, ahead of GRU1, and barrier B2 comes 0.04 µs later
        float q2v[2], p2v[2], bi2[2], ghv[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int gi = ui * 3 + (q == 0 ? gq : 2);
            q2v[q] = cst[XC_Q2 + gi];
            p2v[q] = tr[XT_P2 + gi];
            bi2[q] = cst[XC_BIH2 + gi];
            ghv[q] = gh2s[gi] + cst[XC_BHH2 + gi];
        }
        const float wi0v = cst[XC_WI0 + ui], civ = tr[XT_CI + ui];
        // ---- GRU1 (:208-210), unit tid
        {
            const float r = sigmoid_(fmaf(x, q1r, s4.x));
            const float z = sigmoid_(fmaf(x, q1z, s4.y));
            const float n = tanh_(fmaf(x, q1n, s4.z) + s4.w * r);
            h1v = (h1v - n) * z + n;
            h1s[tid] = h1v;
        }
        float p2q[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) p2q[q] = fmaf(x, q2v[q], p2v[q]) + bi2[q];
        const float xi = fmaf(wi0v, x, civ);   // x_I of unit ui
        bar();
        XSTAMP(1);
        // ---- GRU2 (:212-214) on waves 0, 5..7: the engine's two units, W_ih2[:, :R]·h1 of their six
        // gate rows (two rows per packed FMA: e32part2).  The four r and z rows first, reduce-scattered
        // to lanes 0..3 of the engine (a_r, a_z, b_r, b_z), where one sigmoid pass serves all four;
        // the two n rows and their reduce (a_n → lanes 0, 1, b_n → lanes 2, 3) issue under that
        // pass's exp → rcp chain.  tanh and h' in lanes 0 and 2: r is the lane's own sigmoid, z its
        // neighbour's.  Sums and gate math are gru_gate_math's, operation for operation
        if (g2w) {
            f4v hx[4];
            e32x(h1s, li, hx);
            // x_I + h1 of the lane's unit (:212) formed before the dots and pinned there: hipcc
            // otherwise sinks the h1 LDS read into the publishing lanes' branch after the gate math;
            // the y publish's tag word likewise (a VGPR copy of the step's scalar)
            float yb = xi + h1s[c * kXUnits + ui];
            uint32_t tagv = tag;
            asm volatile("" : "+v"(yb), "+v"(tagv));
            const f2v ga = e32part2(W4x8(0), hx), gb = e32part2(W4x8(8), hx);
            const float g_s = e32rs4(ga.x, ga.y, gb.x, gb.y, lane);
            const float s = sigmoid_(ghv[0] + (g_s + p2q[0]));   // lane 0: r_a, 1: z_a, 2: r_b, 3: z_b
            const f2v gn = e32part2(W4x8(16), hx);
            const float g_n = e32rs2(gn.x, gn.y, lane);
            const float z = WRNN_DPP(s, 0xF5);                   // quad_perm [1,1,3,3]
            const float n = tanh_((g_n + p2q[1]) + ghv[1] * s);
            const float hn = (h2own - n) * z + n;
            h2own = hn;
            // y = (x_I + h1) + h2 (:212, :216); h2: after hop Y (pub_h2)
            pub4(XH_Y, yb + hn, tagv);
            if (wave == 0) set_flag(ypub, tag);
        }
        XSTAMP(2);
        // Off-critical memory traffic (GRU1-term and h2 publishes, the S / h2 gathers, the ring)
        // waits for the critical waves' flags: hop Y's window (GRU2 → y gathered) carries only y,
        // hop F1's only f1, hop F2's only the partials (a second poll stream or a burst of stores
        // beside a critical poll costs it ≈ 0.2 µs: tools/xcdhop.hip PACED variants).
        //   after wave 0's y store : W_hh1·h1 on the fc2 waves (not into GRU2's issue slots on the
        //                            SIMDs they share with waves 7 and 0)
        //   after y gathered  : publish the GRU1 terms of step t+1 and h2 (waves 0, 5..7)
        //   after f1 gathered : gather h2 (wave 6), S (waves 1, 2, 5, then 4), the ring (wave 7)
        //   after h2 gathered : W_hh2·h2 (waves 1..7)
        auto pub_h2 = [&]() { pub4(XH_H2, h2own, tag); };   // GRU2 waves
        // fc waves: lane l ends fc8_rows_rp with row 8h + j + 2·(l >> 4) in o[j]; lanes with
        // (l & 15) < 2 publish row 8h + (l & 1) + 2·(l >> 4)
        const int jq = lane & 1, rho = jq + 2 * (lane >> 4);
        if (wave == 0) {
            if (more && !WRNN_XCD_SKIP_RECUR) {
                float gh[5];
                gh1_dots(gh);
                wait_flag(ygot, tag);
                publish_terms(t + 1, gh);
                pub_h2();
            }
            // ---- hop F2: Σ of the 32 workgroups' partials + b3 → sample
            // lane l: logits (2jp, 2jp+1), jp = l & 15, of producers 8·(l >> 4) + m, m = 0..7:
            // one 16-byte load each (256 B apart: immediates)
            const int jp = lane & 15, pg = lane >> 4;
            const float *nzt = kWin ? NZ(t) : tr + XT_NZ;
            const float ua = nzt[jp < 5 ? 2 * jp : 0], ub = nzt[jp < 5 ? 2 * jp + 1 : 0], u10 = nzt[10];
            const float b3a = cst[XC_B3 + 2 * jp], b3b = cst[XC_B3 + 2 * jp + 1];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // no F2 poll round before fc2 wave 4 has handed its partials to wave 3 (the tag word of its first
            // pair; wave 4 stores on every path): ≈ 0.05 µs before wave 3's publish, ≈ 0.4 µs before the hop
            // can complete, so the poller is in flight when the lines land
            if (WRNN_XCD_F2_GATE) wait_flag(reinterpret_cast<int *>(f2x) + 1, tag);
            const __amdgpu_buffer_rsrc_t rf = hop_rsrc(XG(XH_F2));
            const int goff = pg * 8 * kXF2Line * 8 + jp * 16;
            const unsigned long long c0 = __builtin_amdgcn_s_memrealtime();
            unsigned spins = 0;
            // the polled pieces: a transient of the poll (no GRU2 operand is live here), polled in
            // place and read after the loop (the abort path zeroes them there: no copies on the exit)
            u4v v[8];
            for (;;) {
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = ld16_sc1(rf, goff + m * kXF2Line * 8);
                bool ok = true;
#pragma unroll
                for (int m = 0; m < 8; ++m) ok &= (v[m].y == tag) & (v[m].w == tag);
                if (__ballot(!ok) == 0) break;   // wave-uniform exit: no exec-mask branches
                if ((++spins & 63u) == 0) {
                    const bool late = (long long)(__builtin_amdgcn_s_memrealtime() - c0) > a.timeout_ticks;
                    const bool other = __hip_atomic_load(&a.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                    if (late || other) {
                        if (late) record_abort(a.ctl, -4, t, XH_F2, blockIdx.x);
                        *abort_flag = 1;
#pragma unroll
                        for (int m = 0; m < 8; ++m) v[m] = u4v{0u, 0u, 0u, 0u};
                        break;
                    }
                }
            }
            float pa[8], pb[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                pa[m] = __uint_as_float(v[m].x);
                pb[m] = __uint_as_float(v[m].z);
            }
            XSTAMP(7);
#pragma unroll
            for (int n = 4; n >= 1; n /= 2)
#pragma unroll
                for (int m = 0; m < n; ++m) {
                    pa[m] += pa[m + n];
                    pb[m] += pb[m + n];
                }
            // + the other producer groups (lanes l ^ 16, l ^ 32): identical bits in all four
            cross_rows_pair(pa[0], pb[0]);
            const float la = pa[0] + b3a, lb = pb[0] + b3b;   // logits 2jp, 2jp+1
            x = mol_sample_pairs(la, lb, ua, ub, u10, jp);
            if (lane == 0) {
                xs[t & 1] = x;
                if constexpr (kGrp) {
                    if (c == 0) rw.out[t - rw.out_t0] = x;
                } else {
                    if (c == 0) a.out[kWin ? (size_t)b * a.out_ld + (t - a.out_t0) : (size_t)b * L + t] = x;
                }
            }
            XSTAMP(8);
        } else if (wave < kXWaveFc2) {
            // ---- hop Y → fc1 (:216-218) rows 8h.. in registers → relu → hop F1
            const int hf = wave - kXWaveFc1, rg = 8 * hf + rho;
            const float v1 = tr[XT_V1 + rg];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            u4v v[4];
            xpoll16<4>(XG(XH_Y), tag, a.ctl, a.timeout_ticks, t, XH_Y, abort_flag, lane, v);
            if (hf == 0) set_flag(ygot, tag);
            XSTAMPW(3, 1);
            float o[2];
            fc8_rows_rp(W4x16(), v, o);
            const float A = (jq == 0 ? o[0] : o[1]) + v1;
            if ((lane & 15) < 2) xpub_b(xgr, XGI(XH_F1) + c * kXFcRows + rg, tag, A > 0.0f ? A : 0.0f);
            XSTAMPW(4, 1);
            if (more && !WRNN_XCD_SKIP_RECUR) {   // after f1 gathered: a quarter of the next S; W_hh2 VGPR passes 3h.., LDS passes 15 + 2h..
                wait_flag(f1got, tag);
                if (!WRNN_XCD_SKIP_SG) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    gather_terms(t + 1);
                }
                wait_flag(h2ready, tag);
                f4v hx[4];
                e32x(h2s, li, hx);
                const float gh[5] = {e32dot(W4(16), hx), e32dot(W4(20), hx), e32dot(W4(24), hx), 0.0f, 0.0f};
                gh2_store(6 * hf, 3, gh);
                gh2_lds(15 + 2 * hf, 2, hx);
                XSTAMPW(11, 1);
            }
        } else if (wave < kXWaveFc2 + 2) {
            const int hf = wave - kXWaveFc2;
            if (more && !WRNN_XCD_SKIP_RECUR) {   // W_hh1 rows once GRU2 is through; after y gathered their terms out
                wait_flag(ypub, tag);
                float gh[5];
                gh1_dots(gh);
                wait_flag(ygot, tag);
                publish_terms(t + 1, gh);
            }
            XSTAMPW(9, 3);
            // ---- hop F1 → fc2 (:220-221) rows 8h.. in registers → relu → fc3 partial logits of
            // those rows (:223); wave 4 hands its partials to wave 3 (LDS flag), wave 3 publishes
            // the workgroup's 32 (hop F2)
            float v2[2], w3c[8];
#pragma unroll
            for (int j = 0; j < 2; ++j) v2[j] = tr[XT_V2 + 8 * hf + j + 2 * (lane >> 4)];
#pragma unroll
            for (int r = 0; r < 8; ++r) w3c[r] = w3s[(8 * hf + r) * 32 + li];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            u4v v[4];
            xpoll16<4>(XG(XH_F1), tag, a.ctl, a.timeout_ticks, t, XH_F1, abort_flag, lane, v);
            if (hf == 0) set_flag(f1got, tag);
            XSTAMPW(5, 3);
            float o[2];
            fc8_rows_rp(W4x16(), v, o);
            float p = 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float f = o[j] + v2[j];
                const float f2 = f > 0.0f ? f : 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) p = fmaf(w3c[j + 2 * g], lane_bcast(f2, 16 * g), p);
            }
            // wave 4 → wave 3: 8-byte (value, tag) pairs in LDS, polled by the consumer lanes
            // themselves (one LDS round trip less than data + flag + a flag poll)
            unsigned long long *f2p = reinterpret_cast<unsigned long long *>(f2x);
            if (hf == 1) {
                if (lane < 32)
                    __hip_atomic_store(f2p + lane, ((unsigned long long)tag << 32) | __float_as_uint(p), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                // wave 4 stores on every path (its poll is bounded); the abort word ends the wait
                // too should that ever change
                unsigned spin = 0;
                unsigned long long pv = (unsigned long long)tag << 32;
                for (;;) {
                    if (lane < 32) pv = __hip_atomic_load(f2p + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (__ballot((uint32_t)(pv >> 32) != tag) == 0) break;
                    if ((++spin & 255u) == 0 &&
                        __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
                        break;
                }
                if (lane < kXF2Line)   // 30, 31: zero weights
                    xpub_b(xgr, XGI(XH_F2) + c * kXF2Line + lane, tag, p + __uint_as_float((uint32_t)pv));
                XSTAMPW(6, 3);
            }
            // the fourth quarter of the next step's GRU1 terms (this wave has polled F1 itself:
            // the hop F1 window is over)
            if ((WRNN_XCD_SQ3_WAVE == 3 || WRNN_XCD_SQ3_WAVE == 4) && wave == WRNN_XCD_SQ3_WAVE && more &&
                !WRNN_XCD_SKIP_RECUR && !WRNN_XCD_SKIP_SG) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                gather_terms(t + 1);
            }
            if (more && !WRNN_XCD_SKIP_RECUR) {   // W_hh2 VGPR passes 6 + 3h..; wave 3: LDS passes 22, 23
                wait_flag(h2ready, tag);
                f4v hx[4];
                e32x(h2s, li, hx);
                const float gh[5] = {e32dot(W4(16), hx), e32dot(W4(20), hx), e32dot(W4(24), hx), 0.0f, 0.0f};
                gh2_store(12 + 6 * hf, 3, gh);
                if (hf == 0) gh2_lds(22, 2, hx);
            }
        } else if (more) {
            // ---- waves 5..7: W_hh1 rows (5, 7) → after y gathered their terms and h2 out; after
            // f1 gathered: h2 (wave 6, then flag), an S quarter (5; 6 with WRNN_XCD_SQ3_WAVE 6),
            // the ring (7); after h2 gathered: W_hh2·h2 (VGPR pass 7 + w; LDS pass 19 on wave 5,
            // 20, 21 on wave 6)
            if (WRNN_XCD_SKIP_RECUR) {
                if (wave == 7) {
                    wait_flag(f1got, tag);
                    if (t + 2 >= t0 + 3) {
                        if (t + 2 <= t_terms && lane < kXTerms / 4)
                            reinterpret_cast<f4v *>(RING(t + 2))[lane] = reinterpret_cast<const f4v *>(TERMS(t + 2))[lane];
                        if constexpr (kWin)
                            if (t + 2 < nz_hor && lane < 11) NZ(t + 2)[lane] = noise_term(t + 2);
                    }
                }
                goto step_end;
            }
            if (wave != 6) {
                float gh[5];
                gh1_dots(gh);
                wait_flag(ygot, tag);
                publish_terms(t + 1, gh);
            } else {
                wait_flag(ygot, tag);
            }
            pub_h2();
            wait_flag(f1got, tag);
            if (wave == 6) {
                if (!WRNN_XCD_SKIP_H2) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    xgather16<4>(XG(XH_H2), tag, a.ctl, a.timeout_ticks, t, XH_H2, abort_flag, lane,
                                 [&](int i, float v0, float v1) { *reinterpret_cast<f2v *>(h2s + i) = f2v{v0, v1}; });
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                set_flag(h2ready, tag);
                XSTAMPW(10, 6);
            }
            if (wave <= 6) {
                if (!WRNN_XCD_SKIP_SG && (wave == 5 || WRNN_XCD_SQ3_WAVE == 6)) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    gather_terms(t + 1);
                }
                XSTAMPW(14, 5);
            } else if (t + 2 >= t0 + 3) {
                // ring: step t+2's terms and sampler noise, loaded and stored within this window
                // (a load carried across steps in registers would not fit the VGPR budget, and an
                // LDS-DMA makes hipcc wait for it before every later LDS access of the issuing wave;
                // issued here and stored after the wave's W_hh2 pass: 3.25 -> 3.30 us/step)
                if (t + 2 <= t_terms && lane < kXTerms / 4)
                    reinterpret_cast<f4v *>(RING(t + 2))[lane] = reinterpret_cast<const f4v *>(TERMS(t + 2))[lane];
                if constexpr (kWin)
                    if (t + 2 < nz_hor && lane < 11) NZ(t + 2)[lane] = noise_term(t + 2);
                XSTAMPW(12, 7);
            }
            wait_flag(h2ready, tag);
            {
                f4v hx[4];
                e32x(h2s, li, hx);
                const float gh[5] = {e32dot(W4(24), hx), 0.0f, 0.0f, 0.0f, 0.0f};
                gh2_store(2 * (7 + wave), 1, gh);
                if (wave != 7) gh2_lds(wave == 5 ? 19 : 20, wave == 5 ? 1 : 2, hx);
                XSTAMPW(13, WRNN_XCD_STAMP_W13);
            }
        }
    step_end:
        XSTAMP_BAR();
        bar();
        // next step's x, GRU1 terms and the abort word: one LDS round trip
        const int ab = *abort_flag;
        const float xn = xs[t & 1];
        s4 = lds4(sg + 4 * tid);
        if (ab) return;
        if (wave != 0) x = xn;
        if constexpr (kLst) {
            if (t + 1 == t_end) {
                // ---- the lane's next piece: the state store, then its window, bases and descriptor;
                // the LDS tags back to 0 behind a barrier (the state store was the last reader of the
                // old piece's LDS), ahead of the barrier that follows the new piece's state set-up
                // (the argument stands above the kernel)
                XCD_PIECE_END();
                if (++pi >= pend) return;
                rw = list_piece<XcdRow>(ka.pieces, pi);
                t0 = rw.t0;
                Lc = rw.Lc;
                L = rw.L;
                t_end = t0 + Lc;
                t_terms = min(t_end, L - 1);
                nz_hor = rw.nz_hor;
                xg = rw.xg;
                xgr = __builtin_amdgcn_make_buffer_rsrc(xg, 0, 0x7fffffff, 0x00020000);
                prow = (unsigned long long)rw.row;
                seed = rw.seed;
                __syncthreads();
                if (tid < 64) f2x[tid] = 0.0f;
                if (tid >= 64 && tid < 70) misc[tid - 62] = 0;
                XCD_PIECE_BEGIN();
                t = t0 - 1;
            }
        }
    }
    if constexpr (!kLst) XCD_PIECE_END();
}

#define WRNN_K_XCD fatchord_xcd_kernel<false, false>
#define WRNN_K_XCD_DBG fatchord_xcd_kernel<true, false>
#define WRNN_K_XCD_WIN fatchord_xcd_kernel<false, true>   // streaming sessions (no stamps)
#define WRNN_K_XCD_GRP fatchord_xcd_kernel<false, true, true>   // group pushes: a window per row
#define WRNN_K_XCD_LST fatchord_xcd_kernel<false, true, true, true>   // list launches: a queue of pieces per XCD

// The sampler terms of a one-shot launch (fatchord_xcd.h: launch_xcd_draws): one thread per float of a
// row-step's record, stored to slot XT_NZ of all kXcdWgs workgroup records of that terms row.
// noise_term's two device functions in this file, under this file's flags: the bits the loop formed.
__global__ void xcd_draws_kernel(float *terms, const float *noise, unsigned long long seed, long long row0, int nb, int Bt,
                                 int b0, int t0, int n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * nb * kXNoise) return;
    const int kk = (int)(i % kXNoise), lr = (int)((i / kXNoise) % nb), t = t0 + (int)(i / ((long long)kXNoise * nb));
    float v = 0.0f;
    if (kk < 11) {
        const float uu = noise ? noise[((size_t)t * Bt + b0 + lr) * 11 + kk]
                               : philox_noise(seed, (unsigned long long)(row0 + lr), (uint32_t)t, (uint32_t)kk, 1);
        v = mol_noise_term(uu, kk);
    }
    float *rec = terms + (size_t)(i / kXNoise) * (kXcdWgs * kXTerms) + XT_NZ + kk;
    for (int c = 0; c < kXcdWgs; ++c) rec[(size_t)c * kXTerms] = v;
}

hipError_t launch_xcd_draws(float *terms, const float *noise, unsigned long long seed, long long row0, int nb, int Bt,
                            int b0, int t0, int n, hipStream_t st) {
    const long long m = (long long)n * nb * kXNoise;
    hipLaunchKernelGGL(xcd_draws_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, terms, noise, seed, row0,
                       nb, Bt, b0, t0, n);
    return hipGetLastError();
}

hipError_t launch_xcd(const XcdArgs &a, hipStream_t st) {
    XcdArgs args = a;
    void *params[] = {&args};
    const void *kf = a.windowed ? (const void *)WRNN_K_XCD_WIN : a.dbg ? (const void *)WRNN_K_XCD_DBG : (const void *)WRNN_K_XCD;
    return hipLaunchKernel(kf, dim3(kXcds * kXcdWgs), dim3(kXThreads), params, xcd_lds_layout().total * sizeof(float), st);
}

hipError_t launch_xcd_group(const XcdGroupArgs &g, hipStream_t st) {
    XcdGroupArgs args = g;
    void *params[] = {&args};
    return hipLaunchKernel((const void *)WRNN_K_XCD_GRP, dim3(kXcds * kXcdWgs), dim3(kXThreads), params,
                           xcd_lds_layout().total * sizeof(float), st);
}

hipError_t launch_xcd_list(const XcdListArgs &g, hipStream_t st) {
    XcdListArgs args = g;
    void *params[] = {&args};
    return hipLaunchKernel((const void *)WRNN_K_XCD_LST, dim3(kXcds * kXcdWgs), dim3(kXThreads), params,
                           xcd_lds_layout().total * sizeof(float), st);
}

hipError_t prepare_xcd_kernel(int max_lds_bytes) {
    for (const void *kf : {(const void *)WRNN_K_XCD, (const void *)WRNN_K_XCD_DBG, (const void *)WRNN_K_XCD_WIN,
                           (const void *)WRNN_K_XCD_GRP, (const void *)WRNN_K_XCD_LST}) {
        hipError_t e = hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds_bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t xcd_occupancy(int *blocks_per_cu) {
    int best = 1 << 30;
    for (const void *kf : {(const void *)WRNN_K_XCD, (const void *)WRNN_K_XCD_DBG, (const void *)WRNN_K_XCD_WIN,
                           (const void *)WRNN_K_XCD_GRP, (const void *)WRNN_K_XCD_LST}) {
        int n = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kf, kXThreads, xcd_lds_layout().total * sizeof(float));
        if (e != hipSuccess) return e;
        best = n < best ? n : best;
    }
    *blocks_per_cu = best;
    return hipSuccess;
}

}  // namespace wrnn
