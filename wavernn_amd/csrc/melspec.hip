// melspec.hip — the mel front end (the reference's utils/dsp.py:41-81, melspectrogram) as ONE kernel:
// reflect-indexed framing → periodic-Hann window → real FFT in LDS → |·| → sparse Slaney filterbank →
// 20·log10(max(1e-5, ·)) → normalise and clip.  One workgroup of 256 threads per frame, so a frame's
// value never depends on which other frames share the launch (the chunked and streamed entries rely
// on that for bit-identity).  The definition is DESIGN.md §4.4e (a float64 restatement of librosa's
// published formulas, tests/melspec_ref.py); the tables are built here in float64 and rounded once to
// float32, the kernel computes in float32.
//
// Real FFT of N = n_fft taps: z[n] = x[2n] + i·x[2n + 1] (M = N/2 points), Z = FFT_M(z) by Stockham
// autosort stages (one radix-2 stage first when log2 M is odd, then radix-4), ping-pong between two
// LDS buffers, then X[k] = E[k] + e^{-2πik/N}·O[k] with E / O the even / odd halves recovered from
// Z[k] and conj Z[M − k].  Every twiddle is a table entry (no recurrences).  LDS: re / im planes apart,
// element i at i + (i >> 5), which breaks the power-of-two write strides of the early stages.
//
// Tables (floats; wrnn_melspec_tables), M = n_fft/2:
//   [0, 8)            header: first weighted tap, weighted taps, filterbank weights, 0 …
//   win   [n_fft]     the window zero-padded to n_fft (l = (n_fft − win_length)/2 zeros on the left)
//   twM   [2·M]       (cos, −sin)(2πn/M), n < M
//   twN   [2·(M + 1)] (cos, −sin)(2πk/n_fft), k ≤ M
//   start [n_mels], len [n_mels], off [n_mels]   per band: first bin, bins, offset into w (as floats)
//   w     [Σ len]     the band's non-zero weights, bin-major
// Taps whose window value is zero (the padding, and a Hann window's first sample) are never read:
// a streamed frame is final as soon as its last WEIGHTED sample is in (wrnn_melspec_plan).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "condition.h"
#include "wavernn_amd.h"

namespace wrnn {

constexpr int kMsThreads = 256;
constexpr int kMsHeader = 8;
constexpr int kMsMaxMels = 128;

// one signal's share of a launch: frames [t0, t0 + nt) of a signal whose samples [s0, s0 + ns) are at wav
struct MsJob {
    const float *wav;
    float *mel;
    long long s0, total;   // total < 0: not known yet (no reflection at the right edge)
    int ns, t0, nt, ld;
};

struct MsArgs {
    const float *tab;
    const MsJob *jobs;
    int n_fft, log2m, hop, n_mels;
    float min_db;
};

__device__ __forceinline__ int ms_pad(int i) { return i + (i >> 5); }
__device__ __forceinline__ void ms_swap(float *&a, float *&b) {
    float *t = a;
    a = b, b = t;
}

// tap k of frame t, windowed; the sample index reflects about the signal's ends (edge excluded)
__device__ __forceinline__ float ms_tap(const MsJob &j, const float *__restrict__ win, long long first, int k, int wlo,
                                        int wlen) {
    if (k < wlo || k >= wlo + wlen) return 0.0f;
    long long s = first + k;
    if (s < 0) s = -s;
    if (j.total >= 0 && s >= j.total) s = 2 * (j.total - 1) - s;
    s -= j.s0;
    s = s < 0 ? 0 : (s >= j.ns ? j.ns - 1 : s);   // the host refused windows that miss a sample: never taken
    return j.wav[s] * win[k];
}

__global__ __launch_bounds__(kMsThreads) void melspec_kernel(MsArgs a) {
    extern __shared__ float lds[];
    const MsJob j = a.jobs[blockIdx.y];
    if ((int)blockIdx.x >= j.nt) return;
    const int tid = threadIdx.x;
    const int N = a.n_fft, M = N >> 1, P = M + (M >> 5) + 1;
    const float *__restrict__ tab = a.tab;
    const int wlo = (int)tab[0], wlen = (int)tab[1];
    const float *__restrict__ win = tab + kMsHeader;
    const float2 *__restrict__ twM = reinterpret_cast<const float2 *>(win + N);
    const float2 *__restrict__ twN = twM + M;
    const float *__restrict__ bstart = reinterpret_cast<const float *>(twN + M + 1);
    const float *__restrict__ blen = bstart + a.n_mels;
    const float *__restrict__ boff = blen + a.n_mels;
    const float *__restrict__ bw = boff + a.n_mels;

    float *sr = lds, *si = lds + P, *dr = lds + 2 * P, *di = lds + 3 * P;   // source / destination planes
    const long long t = (long long)j.t0 + blockIdx.x;
    const long long first = t * a.hop - M;
    for (int n = tid; n < M; n += kMsThreads) {
        sr[ms_pad(n)] = ms_tap(j, win, first, 2 * n, wlo, wlen);
        si[ms_pad(n)] = ms_tap(j, win, first, 2 * n + 1, wlo, wlen);
    }
    __syncthreads();

    int Ns = 1;
    if (a.log2m & 1) {   // radix 2, Ns = 1: no twiddle
        const int T = M >> 1;
        for (int q = tid; q < T; q += kMsThreads) {
            const float ar = sr[ms_pad(q)], ai = si[ms_pad(q)];
            const float br = sr[ms_pad(q + T)], bi = si[ms_pad(q + T)];
            dr[ms_pad(2 * q)] = ar + br, di[ms_pad(2 * q)] = ai + bi;
            dr[ms_pad(2 * q + 1)] = ar - br, di[ms_pad(2 * q + 1)] = ai - bi;
        }
        __syncthreads();
        ms_swap(sr, dr), ms_swap(si, di), Ns = 2;
    }
    for (; Ns < M; Ns <<= 2) {
        const int T = M >> 2, step = M / (4 * Ns);
        for (int q = tid; q < T; q += kMsThreads) {
            const int k = q & (Ns - 1);
            float ur[4], ui[4];
            ur[0] = sr[ms_pad(q)], ui[0] = si[ms_pad(q)];
#pragma unroll
            for (int r = 1; r < 4; ++r) {
                const float xr = sr[ms_pad(q + r * T)], xi = si[ms_pad(q + r * T)];
                const float2 w = twM[r * k * step];
                ur[r] = xr * w.x - xi * w.y, ui[r] = xr * w.y + xi * w.x;
            }
            const float t0r = ur[0] + ur[2], t0i = ui[0] + ui[2], t1r = ur[0] - ur[2], t1i = ui[0] - ui[2];
            const float t2r = ur[1] + ur[3], t2i = ui[1] + ui[3], t3r = ur[1] - ur[3], t3i = ui[1] - ui[3];
            const int o = ((q - k) << 2) + k;
            dr[ms_pad(o)] = t0r + t2r, di[ms_pad(o)] = t0i + t2i;
            dr[ms_pad(o + Ns)] = t1r + t3i, di[ms_pad(o + Ns)] = t1i - t3r;
            dr[ms_pad(o + 2 * Ns)] = t0r - t2r, di[ms_pad(o + 2 * Ns)] = t0i - t2i;
            dr[ms_pad(o + 3 * Ns)] = t1r - t3i, di[ms_pad(o + 3 * Ns)] = t1i + t3r;
        }
        __syncthreads();
        ms_swap(sr, dr), ms_swap(si, di);
    }

    // |X[k]|, k ≤ M, from Z[k] and conj Z[M − k] → the free buffer's real plane, unpadded
    float *mag = dr;
    for (int k = tid; k <= M; k += kMsThreads) {
        const int k0 = k & (M - 1), k1 = (M - k) & (M - 1);
        const float ar = sr[ms_pad(k0)], ai = si[ms_pad(k0)];
        const float br = sr[ms_pad(k1)], bi = -si[ms_pad(k1)];
        const float er = 0.5f * (ar + br), ei = 0.5f * (ai + bi);
        const float orr = 0.5f * (ai - bi), oi = -0.5f * (ar - br);
        const float2 w = twN[k];
        const float xr = er + orr * w.x - oi * w.y, xi = ei + orr * w.y + oi * w.x;
        mag[k] = sqrtf(xr * xr + xi * xi);
    }
    __syncthreads();

    // filterbank: 16 lanes per band, 16 bands at a time; the lanes' partial sums meet in a fixed order
    const int g = tid >> 4, l = tid & 15;
    for (int b0 = 0; b0 < a.n_mels; b0 += 16) {
        const int b = b0 + g;
        const bool live = b < a.n_mels;
        const int s0 = live ? (int)bstart[b] : 0, n = live ? (int)blen[b] : 0, off = live ? (int)boff[b] : 0;
        float s = 0.0f;
        for (int i = l; i < n; i += 16) s = fmaf(bw[off + i], mag[s0 + i], s);
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m, 16);
        if (live && l == 0) {
            const float db = 20.0f * log10f(fmaxf(1e-5f, s));
            const float v = (db - a.min_db) / -a.min_db;
            j.mel[(size_t)b * j.ld + blockIdx.x] = fminf(fmaxf(v, 0.0f), 1.0f);
        }
    }
}

namespace {

constexpr double kPi = 3.14159265358979323846;

int ms_log2(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

// WRNN_OK, or why the geometry is refused (decided without a launch)
int ms_check(const wrnn_melspec_cfg *c) {
    if (!c) return cond_fail(WRNN_EINVAL, "melspec: null config");
    if (c->sample_rate < 1 || c->n_fft < 1 || c->num_mels < 1 || !(c->min_level_db < 0.0f))
        return cond_fail(WRNN_EINVAL, "melspec: sample_rate, n_fft, num_mels must be positive and min_level_db negative");
    if (c->n_fft < 256 || c->n_fft > 4096 || (c->n_fft & (c->n_fft - 1)))
        return cond_fail(WRNN_EUNSUPPORTED, "melspec: n_fft must be a power of two in 256..4096");
    if (c->win_length < 1 || c->win_length > c->n_fft)
        return cond_fail(WRNN_EUNSUPPORTED, "melspec: win_length must be in 1..n_fft");
    if (c->hop_length < 1) return cond_fail(WRNN_EUNSUPPORTED, "melspec: hop_length must be at least 1");
    if (c->num_mels > kMsMaxMels) return cond_fail(WRNN_EUNSUPPORTED, "melspec: at most 128 mel bands");
    if (!(c->fmin >= 0.0f) || !(2.0 * c->fmin < (double)c->sample_rate))
        return cond_fail(WRNN_EUNSUPPORTED, "melspec: fmin must be in [0, sample_rate/2)");
    return WRNN_OK;
}

// the window zero-padded to n_fft, float64
std::vector<double> ms_window(const wrnn_melspec_cfg *c) {
    std::vector<double> w(c->n_fft, 0.0);
    const int l = (c->n_fft - c->win_length) / 2;
    for (int n = 0; n < c->win_length; ++n) w[l + n] = 0.5 - 0.5 * std::cos(2.0 * kPi * n / c->win_length);
    return w;
}

// [lo, lo + len): the taps whose float32 window value is not zero
void ms_support(const wrnn_melspec_cfg *c, int *lo, int *len) {
    thread_local wrnn_melspec_cfg last{};
    thread_local int last_lo = 0, last_len = -1;
    if (last_len < 0 || std::memcmp(&last, c, sizeof last)) {
        const std::vector<double> w = ms_window(c);
        int a = 0, b = c->n_fft;
        while (a < b && (float)w[a] == 0.0f) ++a;
        while (b > a && (float)w[b - 1] == 0.0f) --b;
        last = *c, last_lo = a, last_len = b - a;
    }
    *lo = last_lo, *len = last_len;
}

double ms_hz_to_mel(double f) {
    return f < 1000.0 ? f / (200.0 / 3.0) : 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0);
}

double ms_mel_to_hz(double m) {
    return m < 15.0 ? (200.0 / 3.0) * m : 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0));
}

// the Slaney filterbank, sparse: per band its first non-zero bin, its bins, and the weights (float64)
void ms_basis(const wrnn_melspec_cfg *c, std::vector<int> *start, std::vector<int> *len, std::vector<double> *w) {
    const int B = c->num_mels, K = c->n_fft / 2 + 1;
    const double lo = ms_hz_to_mel(c->fmin), hi = ms_hz_to_mel(0.5 * c->sample_rate);
    std::vector<double> mf(B + 2);
    const double mstep = (hi - lo) / (B + 1);
    for (int i = 0; i < B + 2; ++i) mf[i] = ms_mel_to_hz(i == B + 1 ? hi : i * mstep + lo);
    const double fstep = 0.5 * c->sample_rate / (K - 1);
    start->assign(B, 0), len->assign(B, 0), w->clear();
    std::vector<double> row(K);
    for (int i = 0; i < B; ++i) {
        const double enorm = 2.0 / (mf[i + 2] - mf[i]);
        int a = K, b = 0;
        for (int k = 0; k < K; ++k) {
            const double f = k == K - 1 ? 0.5 * c->sample_rate : k * fstep;
            const double v = std::max(0.0, std::min((f - mf[i]) / (mf[i + 1] - mf[i]), (mf[i + 2] - f) / (mf[i + 2] - mf[i + 1])));
            row[k] = v * enorm;
            if (row[k] > 0.0) a = std::min(a, k), b = k + 1;
        }
        if (b > a) {
            (*start)[i] = a, (*len)[i] = b - a;
            w->insert(w->end(), row.begin() + a, row.begin() + b);
        }
    }
}

long long ms_frames(const wrnn_melspec_cfg *c, long long n) { return 1 + n / c->hop_length; }

// the samples frames [t0, t0 + nt) read, reflection included: [*lo, *hi]; total < 0: no right reflection
void ms_needed(const wrnn_melspec_cfg *c, int wlo, int wlen, long long total, long long t0, long long nt, long long *lo,
               long long *hi) {
    const long long half = c->n_fft / 2;
    const long long jlo = t0 * c->hop_length + wlo - half, jhi = (t0 + nt - 1) * c->hop_length + wlo + wlen - 1 - half;
    long long a = std::max(jlo, 0LL), b = jhi;
    if (jlo < 0) a = 0, b = std::max(b, -jlo);
    if (total >= 0 && jhi >= total) {
        a = std::min(a, 2 * (total - 1) - jhi);
        b = std::max(std::min(b, total - 1), jlo < 0 ? -jlo : 0LL);
    }
    *lo = a, *hi = b;
}

int ms_launch(const wrnn_melspec_cfg *c, const float *tables, std::vector<MsJob> &jobs, void *scratch, void *stream) {
    int wlo = 0, wlen = 0, max_nt = 0;
    ms_support(c, &wlo, &wlen);
    for (size_t u = 0; u < jobs.size(); ++u) {
        const MsJob &j = jobs[u];
        const std::string at = "melspec: signal " + std::to_string(u) + ": ";
        if (!j.wav || !j.mel || j.ns < 1 || j.s0 < 0 || j.t0 < 0 || j.nt < 0 || j.ld < j.nt)
            return cond_fail(WRNN_EINVAL, at + "null pointer, empty window, or ld below the frame count");
        if (j.total >= 0) {
            if (j.total < c->n_fft / 2 + 1)
                return cond_fail(WRNN_EINVAL, at + "shorter than n_fft/2 + 1 samples (the reflect padding's limit)");
            if (j.s0 + j.ns > j.total || (long long)j.t0 + j.nt > ms_frames(c, j.total))
                return cond_fail(WRNN_EINVAL, at + "window or frames beyond the signal's end");
        }
        if (j.nt && wlen) {
            long long lo = 0, hi = 0;
            ms_needed(c, wlo, wlen, j.total, j.t0, j.nt, &lo, &hi);
            if (lo < j.s0 || hi >= j.s0 + j.ns)
                return cond_fail(WRNN_EINVAL, at + "frames " + std::to_string(j.t0) + ".." + std::to_string(j.t0 + j.nt - 1) +
                                                  " read samples " + std::to_string(lo) + ".." + std::to_string(hi) +
                                                  ", resident are " + std::to_string(j.s0) + ".." +
                                                  std::to_string(j.s0 + j.ns - 1));
        }
        max_nt = std::max(max_nt, j.nt);
    }
    if (!max_nt) return WRNN_OK;
    hipStream_t st = (hipStream_t)stream;
    // `jobs` is pageable and dies with the caller's frame: HIP stages such a copy before it returns,
    // which is what makes this safe and why the header says the call may wait on the stream
    if (hipMemcpyAsync(scratch, jobs.data(), jobs.size() * sizeof(MsJob), hipMemcpyHostToDevice, st) != hipSuccess)
        return cond_fail(WRNN_EHIP, "melspec: copying the job list failed");
    const int M = c->n_fft / 2;
    MsArgs a{tables, (const MsJob *)scratch, c->n_fft, ms_log2(M), c->hop_length, c->num_mels, c->min_level_db};
    const size_t lds = 4 * (size_t)(M + (M >> 5) + 1) * sizeof(float);
    hipLaunchKernelGGL(melspec_kernel, dim3(max_nt, (unsigned)jobs.size()), dim3(kMsThreads), lds, st, a);
    return hipGetLastError() == hipSuccess ? WRNN_OK : cond_fail(WRNN_EHIP, "melspec: launch failed");
}

}  // namespace
}  // namespace wrnn

extern "C" {

static_assert(sizeof(wrnn::MsJob) <= WRNN_MELSPEC_SCRATCH_PER_SIGNAL, "scratch bytes per signal");

int64_t wrnn_melspec_frames(const wrnn_melspec_cfg *cfg, int64_t n_samples) {
    using namespace wrnn;
    if (int rc = ms_check(cfg)) return rc;
    if (n_samples < cfg->n_fft / 2 + 1)
        return cond_fail(WRNN_EINVAL, "melspec: a signal shorter than n_fft/2 + 1 samples cannot be reflect-padded");
    return ms_frames(cfg, n_samples);
}

int wrnn_melspec_table_floats(const wrnn_melspec_cfg *cfg) {
    using namespace wrnn;
    if (int rc = ms_check(cfg)) return rc;
    std::vector<int> start, len;
    std::vector<double> w;
    ms_basis(cfg, &start, &len, &w);
    const int M = cfg->n_fft / 2;
    return kMsHeader + cfg->n_fft + 2 * M + 2 * (M + 1) + 3 * cfg->num_mels + (int)w.size();
}

int wrnn_melspec_tables(const wrnn_melspec_cfg *cfg, float *out) {
    using namespace wrnn;
    if (int rc = ms_check(cfg)) return rc;
    if (!out) return cond_fail(WRNN_EINVAL, "melspec: null table buffer");
    std::vector<int> start, len;
    std::vector<double> w;
    ms_basis(cfg, &start, &len, &w);
    int wlo = 0, wlen = 0;
    ms_support(cfg, &wlo, &wlen);
    const int N = cfg->n_fft, M = N / 2, B = cfg->num_mels;
    float *p = out;
    std::fill(p, p + kMsHeader, 0.0f);
    p[0] = (float)wlo, p[1] = (float)wlen, p[2] = (float)w.size();
    p += kMsHeader;
    for (double v : ms_window(cfg)) *p++ = (float)v;
    for (int n = 0; n < M; ++n) *p++ = (float)std::cos(2.0 * kPi * n / M), *p++ = (float)-std::sin(2.0 * kPi * n / M);
    for (int k = 0; k <= M; ++k) *p++ = (float)std::cos(2.0 * kPi * k / N), *p++ = (float)-std::sin(2.0 * kPi * k / N);
    for (int i = 0; i < B; ++i) *p++ = (float)start[i];
    for (int i = 0; i < B; ++i) *p++ = (float)len[i];
    int off = 0;
    for (int i = 0; i < B; ++i) *p++ = (float)off, off += len[i];
    for (double v : w) *p++ = (float)v;
    return WRNN_OK;
}

int wrnn_melspec_plan(const wrnn_melspec_cfg *cfg, int64_t received, int final, int64_t *frames_ready, int64_t *keep_from) {
    using namespace wrnn;
    if (int rc = ms_check(cfg)) return rc;
    if (received < 0 || !frames_ready || !keep_from) return cond_fail(WRNN_EINVAL, "melspec plan: bad arguments");
    if (final) {
        if (received < cfg->n_fft / 2 + 1)
            return cond_fail(WRNN_EINVAL, "melspec: a signal shorter than n_fft/2 + 1 samples cannot be reflect-padded");
        *frames_ready = ms_frames(cfg, received), *keep_from = received;
        return WRNN_OK;
    }
    int wlo = 0, wlen = 0;
    ms_support(cfg, &wlo, &wlen);
    const long long half = cfg->n_fft / 2, hop = cfg->hop_length;
    // frame t reads up to sample t·hop + (wlo + wlen − 1 − half), and, reflected about sample 0,
    // sample −(t·hop + wlo − half): final once both are in.
    long long t = received / hop + 1;   // never a frame whose centre is not in yet
    if (wlen) {
        const long long right = wlo + wlen - half;   // frame t is in once received ≥ t·hop + right
        if (right > 0) t = received >= right ? std::min(t, (received - right) / hop + 1) : 0;
        // frame 0 mirrors the most, and no frame is ready before frame 0
        if (wlo < half && received < half - wlo + 1) t = 0;
    }
    *frames_ready = t;
    // the next frame's first weighted sample, or, one less than its mirror image should the signal
    // end right at that frame's centre (the earliest end at which the frame exists)
    const long long c = t * hop;
    *keep_from = std::max(0LL, std::min(c + wlo - half, c - 1 - (wlo + wlen - half)));
    if (*keep_from > received) *keep_from = received;
    return WRNN_OK;
}

int wrnn_melspec_windows(const wrnn_melspec_cfg *cfg, const float *tables, const float *const *wav_tail, const int64_t *s0,
                         const int *ns, const int64_t *total, const int *t0, const int *nt, int U, float *const *mel,
                         const int *ld, void *scratch, void *stream) {
    using namespace wrnn;
    if (int rc = ms_check(cfg)) return rc;
    if (!tables || !wav_tail || !s0 || !ns || !total || !t0 || !nt || !mel || !ld || !scratch || U < 1 || U > 65535)
        return cond_fail(WRNN_EINVAL, "melspec: null argument or U outside 1..65535");
    std::vector<MsJob> jobs(U);
    for (int u = 0; u < U; ++u) jobs[u] = MsJob{wav_tail[u], mel[u], s0[u], total[u] < 0 ? -1 : total[u], ns[u], t0[u], nt[u], ld[u]};
    return ms_launch(cfg, tables, jobs, scratch, stream);
}

int wrnn_melspec(const wrnn_melspec_cfg *cfg, const float *tables, const float *const *wav, const int *n, int U,
                 float *const *mel, const int *ld, void *scratch, void *stream) {
    using namespace wrnn;
    if (int rc = ms_check(cfg)) return rc;
    if (!tables || !wav || !n || !mel || !ld || !scratch || U < 1 || U > 65535)
        return cond_fail(WRNN_EINVAL, "melspec: null argument or U outside 1..65535");
    std::vector<MsJob> jobs(U);
    for (int u = 0; u < U; ++u) {
        if (n[u] < cfg->n_fft / 2 + 1)
            return cond_fail(WRNN_EINVAL, "melspec: signal " + std::to_string(u) + " is shorter than n_fft/2 + 1 samples");
        jobs[u] = MsJob{wav[u], mel[u], 0, n[u], n[u], 0, (int)ms_frames(cfg, n[u]), ld[u]};
    }
    return ms_launch(cfg, tables, jobs, scratch, stream);
}

int wrnn_melspec_window(const wrnn_melspec_cfg *cfg, const float *tables, const float *wav_tail, int64_t s0, int ns,
                        int64_t total, int t0, int nt, float *mel, int ld, void *scratch, void *stream) {
    return wrnn_melspec_windows(cfg, tables, &wav_tail, &s0, &ns, &total, &t0, &nt, 1, &mel, &ld, scratch, stream);
}

}  // extern "C"
