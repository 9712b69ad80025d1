// opt_wide.hip -- the optimiser for evaluations the CALLER supplies, for problems of up to 32768 variables: sfx_opt_wide_*
// (include/sfx.h).
//
// Replaces, for B independent problems whose loss and gradient come from outside the library:
//   FittingMonitor.run_fitting          smplifyx/fitting.py:147-217            (mode 0)
//   LBFGS.step                          smplifyx/optimizers/lbfgs_ls.py:256-445 (mode 1)
//   _strong_Wolfe / _cubic_interpolate  smplifyx/optimizers/lbfgs_ls.py:11-167
// The state machine is lbfgs_wide.h over the scalar transitions of lbfgs_scalar.h, which the fit loop's tick shares (specification:
// oracle/lbfgs_machine.py); this file is its vector layer for ONE WORKGROUP of 1024 threads per problem, the kernel that consumes
// one evaluation per launch, and the C ABI, whose host half shared with sfx_opt_* is opt_host.h.
//
// Layout.  A row is N floats padded with zeros to a multiple of 4; thread t owns its 16-byte chunks t, t + 1024, ... (at most 8
// at N = 32768), in every row alike: element-wise work needs no barrier, a thread only ever reads what it wrote itself.  The
// working rows and the history ring live in device memory (they stay in L2 / Infinity Cache between launches); the vector of
// the two-loop recursion lives in registers.
// Arithmetic.  A dot product is accumulated in float64 by each thread over its chunks in order, then over the wavefront
// (butterfly), then over the 16 wavefronts' partial sums in order, and rounded to float32 once: the arithmetic of
// tests/opt_ext_common.Dot64Machine up to the order of exact-to-2^-53 additions.  No atomics; a problem's bits depend on
// its own inputs only.
// Who does what.  The machine is scalar code over a 360-byte state: 1024 private copies of it do not fit the register file
// (128 VGPRs per thread at this workgroup size), so wavefront 0 alone runs it, on the state in LDS, and POSTS each vector
// operation to the workgroup through a two-slot command buffer: one workgroup barrier per operation, two per reduction.  The
// axpy of a recursion step rides with the next step's dot product, so a step of the two-loop recursion costs two barriers.
#include "../../include/sfx.h"
#include "sfx_internal.h"
#include "lbfgs_wide.h"
#include "opt_host.h"

#include <memory>
#include <vector>

#pragma clang fp contract(off)

#define WIDE_THREADS 1024
#define WIDE_WAVES (WIDE_THREADS / 64)
#define WIDE_CHUNKS (SFX_WIDE_NMAX / 4 / WIDE_THREADS)      // 16-byte chunks of a row per thread, at most
#define WIDE_RO (SFX_HIST_MAX + 4)                           // the ring has history_size + 1 slots
static_assert(WIDE_CHUNKS == 8, "a thread holds 32 elements of a row at the cap");

struct WideDev {
    WideCfg cfg;               // (g_off / g_len: device pointers)
    int B, Np;                 // Np: floats per row, N rounded up to a multiple of 4
    float* rows;               // [B][W_NROWS][Np]
    float* hist;               // [B][2][history_size + 1][Np]: y rows, then s rows
    float* ro;                 // [B][WIDE_RO]
    WideState* st;             // [B]
    int* status;               // [B] (what sfx_opt_wide_active reads)
    float4* trace; int* trace_n; int trace_cap;
};

// What wavefront 0 asks the workgroup to do: one vector operation over every thread's own chunks.
enum { OP_EXIT = 0, OP_DOTS, OP_AXPY, OP_COPY, OP_NEG, OP_SUB, OP_SCALE, OP_ASUM, OP_AMAXS, OP_GMAX, OP_RLOADNEG, OP_RDOT, OP_RSCALE, OP_RSTORE };
struct WCmd {
    int op, n, off, len;
    float f, pf;               // pf, py: an axpy on the register vector that is still owed (q += pf * py), done first by the R operations
    float* dst;
    const float *a, *b, *a1, *b1, *py;
};

#define WIDE_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)

// One thread's share of the vector work: its chunks of the rows, its chunks of the register vector.
struct WgWork {
    const unsigned nch, tid;   // unsigned: a row is addressed as (uniform base) + (32-bit offset of this thread's chunk)
    double* const s_part;      // [2][WIDE_WAVES] the wavefronts' partial results of a reduction
    // the register vector q: chunk j of thread t is chunk t + 1024 j of a row (statically indexed: it stays in registers)
    typedef float4 Q[WIDE_CHUNKS];

    static __device__ float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
    template <class T> static __device__ T* uni(T* p) {
        const unsigned long long u = reinterpret_cast<unsigned long long>(p);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
        return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
    }
    static __device__ const float4* c4(const float* p) { return reinterpret_cast<const float4*>(p); }
    static __device__ float4* m4(float* p) { return reinterpret_cast<float4*>(p); }
    static __device__ void fma4(double& acc, const float4 a, const float4 b) {
        acc = acc + (double)a.x * (double)b.x; acc = acc + (double)a.y * (double)b.y;
        acc = acc + (double)a.z * (double)b.z; acc = acc + (double)a.w * (double)b.w;
    }
    static __device__ float4 axpy4(const float4 x, const float a, const float4 y) {
        return make_float4(fmaf(a, y.x, x.x), fmaf(a, y.y, x.y), fmaf(a, y.z, x.z), fmaf(a, y.w, x.w));
    }
    // this thread's partial result -> its wavefront's (butterfly, a fixed order), left in s_part[r][wave]
    template <bool MAX> __device__ void wave_part(double a, int r) const {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const double p = __shfl_xor(a, o, 64); a = MAX ? fmax(a, p) : a + p; }
        if ((tid & 63) == 0) s_part[r * WIDE_WAVES + (tid >> 6)] = a;
    }
    __device__ void owed_axpy(const WCmd& c, Q& q, const unsigned t) const {
        if (!c.py) return;
#pragma unroll
        for (int j = 0; j < WIDE_CHUNKS; ++j) { const unsigned k = t + j * WIDE_THREADS; if (k < nch) q[j] = axpy4(q[j], c.pf, c4(c.py)[k]); }
    }
    // Returns true for a reduction: the partial results are in s_part, a barrier away from being read.
    __device__ bool exec(const WCmd& c, Q& q) const {
        // The thread's chunk index, made opaque once per operation: the state machine around the operations is a loop, and with a
        // loop-invariant index the compiler keeps every (row, chunk) address of every operation alive in registers across it.
        unsigned t = tid;
        asm volatile("" : "+v"(t));
        switch (c.op) {
        case OP_DOTS: {
            double a0 = 0.0, a1 = 0.0;
            if (c.n == 2) for (unsigned k = t; k < nch; k += WIDE_THREADS) { fma4(a0, c4(c.a)[k], c4(c.b)[k]); fma4(a1, c4(c.a1)[k], c4(c.b1)[k]); }
            else for (unsigned k = t; k < nch; k += WIDE_THREADS) fma4(a0, c4(c.a)[k], c4(c.b)[k]);
            wave_part<false>(a0, 0);
            if (c.n == 2) wave_part<false>(a1, 1);
            return true;
        }
        case OP_AXPY: for (unsigned k = t; k < nch; k += WIDE_THREADS) m4(c.dst)[k] = axpy4(c4(c.a)[k], c.f, c4(c.b)[k]); return false;
        case OP_COPY: for (unsigned k = t; k < nch; k += WIDE_THREADS) m4(c.dst)[k] = c4(c.a)[k]; return false;
        case OP_NEG:
            for (unsigned k = t; k < nch; k += WIDE_THREADS) { const float4 v = c4(c.a)[k]; m4(c.dst)[k] = make_float4(-v.x, -v.y, -v.z, -v.w); }
            return false;
        case OP_SUB:
            for (unsigned k = t; k < nch; k += WIDE_THREADS) {
                const float4 u = c4(c.a)[k], w = c4(c.b)[k];
                m4(c.dst)[k] = make_float4(u.x - w.x, u.y - w.y, u.z - w.z, u.w - w.w);
            }
            return false;
        case OP_SCALE:
            for (unsigned k = t; k < nch; k += WIDE_THREADS) { const float4 v = c4(c.a)[k]; m4(c.dst)[k] = make_float4(v.x * c.f, v.y * c.f, v.z * c.f, v.w * c.f); }
            return false;
        case OP_ASUM: {
            double a0 = 0.0;
            for (unsigned k = t; k < nch; k += WIDE_THREADS) {
                const float4 v = c4(c.a)[k];
                a0 = a0 + fabs((double)v.x); a0 = a0 + fabs((double)v.y); a0 = a0 + fabs((double)v.z); a0 = a0 + fabs((double)v.w);
            }
            wave_part<false>(a0, 0);
            return true;
        }
        case OP_AMAXS: {
            float m = 0.f;
            for (unsigned k = t; k < nch; k += WIDE_THREADS) {
                const float4 v = c4(c.a)[k];
                m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x * c.f), fabsf(v.y * c.f)), fmaxf(fabsf(v.z * c.f), fabsf(v.w * c.f))));
            }
            wave_part<true>((double)m, 0);
            return true;
        }
        case OP_GMAX: {
            float m = -INFINITY;
            for (unsigned k = t; k < nch; k += WIDE_THREADS) {
                const int e0 = (int)(4 * k);
                if (e0 + 3 < c.off || e0 >= c.off + c.len) continue;
                const float4 v = c4(c.a)[k];
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) if (e0 + i >= c.off && e0 + i < c.off + c.len) m = fmaxf(m, e[i]);
            }
            wave_part<true>((double)m, 0);
            return true;
        }
        case OP_RLOADNEG:
#pragma unroll
            for (int j = 0; j < WIDE_CHUNKS; ++j) {
                const unsigned k = t + j * WIDE_THREADS;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < nch) v = c4(c.a)[k];
                q[j] = make_float4(-v.x, -v.y, -v.z, -v.w);
            }
            return false;
        case OP_RDOT: {
            owed_axpy(c, q, t);
            double a0 = 0.0;
#pragma unroll
            for (int j = 0; j < WIDE_CHUNKS; ++j) { const unsigned k = t + j * WIDE_THREADS; if (k < nch) fma4(a0, q[j], c4(c.a)[k]); }
            wave_part<false>(a0, 0);
            return true;
        }
        case OP_RSCALE:
            owed_axpy(c, q, t);
#pragma unroll
            for (int j = 0; j < WIDE_CHUNKS; ++j) { const float4 v = q[j]; q[j] = make_float4(v.x * c.f, v.y * c.f, v.z * c.f, v.w * c.f); }
            return false;
        case OP_RSTORE:
            owed_axpy(c, q, t);
#pragma unroll
            for (int j = 0; j < WIDE_CHUNKS; ++j) { const unsigned k = t + j * WIDE_THREADS; if (k < nch) m4(c.dst)[k] = q[j]; }
            return false;
        default: return false;
        }
    }
    // wavefronts 1..15: do what wavefront 0 posts until it says stop (command i sits in slot i & 1: one barrier per command)
    __device__ void serve(const WCmd* s_cmd) const {
        Q q;
        for (int i = 0;; ++i) {
            __syncthreads();
            WCmd c = s_cmd[i & 1];
            // (every field is the same in all lanes: say so, and the rows are addressed from scalar registers as in wavefront 0)
            c.op = __builtin_amdgcn_readfirstlane(c.op); c.n = __builtin_amdgcn_readfirstlane(c.n);
            c.off = __builtin_amdgcn_readfirstlane(c.off); c.len = __builtin_amdgcn_readfirstlane(c.len);
            c.f = uni(c.f); c.pf = uni(c.pf);
            c.dst = uni(c.dst); c.a = uni(c.a); c.b = uni(c.b); c.a1 = uni(c.a1); c.b1 = uni(c.b1); c.py = uni(c.py);
            if (c.op == OP_EXIT) return;
            if (exec(c, q)) __syncthreads();
        }
    }
};

// The machine's vector layer on the device, as wavefront 0 sees it: every operation is posted to the workgroup, done by all
// 1024 threads (these 64 included), and a reduction's result comes back to the 64 lanes, which all hold the same scalars.
struct WgLayer {
    typedef float* Row;
    struct Reg { WgWork::Q q; };      // wavefront 0's share of the register vector: alive for one recursion only
    const WgWork& w;
    WCmd* const s_cmd;
    OptScal* const s_state;
    float* const s_al; float* const s_ro;
    float* const rows_; float* const hist_;
    const size_t Np;
    const int slots, b;
    float4* const tr; int* const tr_n; const int tr_cap;
    int n_cmd = 0;
    Reg none;                  // (what an operation that does not touch the register vector is handed: never read or written)
    float owed_f = 0.f; const float* owed_y = nullptr;

    __device__ Row row(int k) const { return rows_ + (size_t)k * Np; }
    __device__ Row hist_y(int slot) const { return hist_ + (size_t)slot * Np; }
    __device__ Row hist_s(int slot) const { return hist_ + (size_t)(slots + slot) * Np; }
    __device__ OptScal& scal() const { return *s_state; }
    __device__ float* al() const { return s_al; }
    __device__ float* ro() const { return s_ro; }
    __device__ bool leader() const { return w.tid == 0; }
    __device__ void sync() const { WIDE_WSYNC(); }
    __device__ void trace(int ty, double a, double b_, double c) const {
        if (tr && tr_n && w.tid == 0) {
            const int n = tr_n[b];
            if (n < tr_cap) tr[(size_t)b * tr_cap + n] = make_float4((float)ty, (float)a, (float)b_, (float)c);
            tr_n[b] = n + 1;
        }
    }
    // post, let everybody see it, do this wavefront's share; a reduction's results (n of them) are summed over the wavefronts in order
    __device__ void run(WCmd c, Reg& reg, int n_out = 0, float* out = nullptr, bool max = false) {
        const bool r_op = c.op >= OP_RDOT;
        c.pf = r_op ? owed_f : 0.f; c.py = r_op ? owed_y : nullptr;
        if (r_op || c.op == OP_RLOADNEG) { owed_f = 0.f; owed_y = nullptr; }
        if (w.tid == 0) s_cmd[n_cmd & 1] = c;
        ++n_cmd;
        __syncthreads();
        if (!w.exec(c, reg.q)) return;
        __syncthreads();
        for (int r = 0; r < n_out; ++r) {
            const double* p = w.s_part + r * WIDE_WAVES;
            double acc = p[0];
#pragma unroll
            for (int i = 1; i < WIDE_WAVES; ++i) acc = max ? fmax(acc, p[i]) : acc + p[i];
            out[r] = (float)acc;
        }
    }
    static __device__ WCmd cmd(int op) { WCmd c{}; c.op = op; return c; }
    __device__ void dots(int n, const Row* a, const Row* b_, float* out) {
        WCmd c = cmd(OP_DOTS); c.n = n; c.a = a[0]; c.b = b_[0]; c.a1 = n > 1 ? a[1] : nullptr; c.b1 = n > 1 ? b_[1] : nullptr;
        run(c, none, n, out);
    }
    __device__ float dot(Row a, Row b_) { float r; dots(1, &a, &b_, &r); return r; }
    __device__ void axpy(Row dst, Row x, float a, Row y) { WCmd c = cmd(OP_AXPY); c.dst = dst; c.a = x; c.f = a; c.b = y; run(c, none); }
    __device__ void copy(Row dst, Row src) { WCmd c = cmd(OP_COPY); c.dst = dst; c.a = src; run(c, none); }
    __device__ void neg(Row dst, Row src) { WCmd c = cmd(OP_NEG); c.dst = dst; c.a = src; run(c, none); }
    __device__ void sub(Row dst, Row a, Row b_) { WCmd c = cmd(OP_SUB); c.dst = dst; c.a = a; c.b = b_; run(c, none); }
    __device__ void scale(Row dst, Row a, float f) { WCmd c = cmd(OP_SCALE); c.dst = dst; c.a = a; c.f = f; run(c, none); }
    __device__ float asum(Row a) { WCmd c = cmd(OP_ASUM); c.a = a; float r; run(c, none, 1, &r); return r; }
    __device__ float amax_scaled(Row a, float f) { WCmd c = cmd(OP_AMAXS); c.a = a; c.f = f; float r; run(c, none, 1, &r, true); return r; }
    __device__ float amax(Row a) { return amax_scaled(a, 1.0f); }
    __device__ float gmax(Row a, int off, int len) { WCmd c = cmd(OP_GMAX); c.a = a; c.off = off; c.len = len; float r; run(c, none, 1, &r, true); return r; }
    __device__ void r_load_neg(Reg& q, Row a) { WCmd c = cmd(OP_RLOADNEG); c.a = a; run(c, q); }
    __device__ float r_dot(Reg& q, Row a) { WCmd c = cmd(OP_RDOT); c.a = a; float r; run(c, q, 1, &r); return r; }
    // owed until the next operation on the register vector, which does it first: one barrier saved per step of the recursion
    __device__ void r_axpy(Reg& q, float a, Row y) { if (owed_y) { WCmd c = cmd(OP_RSCALE); c.f = 1.0f; run(c, q); } owed_f = a; owed_y = y; }
    __device__ void r_scale(Reg& q, float f) { WCmd c = cmd(OP_RSCALE); c.f = f; run(c, q); }
    __device__ void r_store(Row dst, Reg& q) { WCmd c = cmd(OP_RSTORE); c.dst = dst; run(c, q); }
    __device__ void stop() { run(cmd(OP_EXIT), none); }
};

// a packed row of the caller (N floats, any alignment) <-> a padded row of the machine, each thread its own chunks
__device__ __forceinline__ void wide_row_in(float* __restrict__ dst, const float* __restrict__ src, int N, int nch, int tid) {
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    for (int c = tid; c < nch; c += WIDE_THREADS) {
        float4 v;
        if (vec) v = reinterpret_cast<const float4*>(src)[c];
        else {
            const int i = 4 * c;
            v.x = src[i]; v.y = i + 1 < N ? src[i + 1] : 0.f; v.z = i + 2 < N ? src[i + 2] : 0.f; v.w = i + 3 < N ? src[i + 3] : 0.f;
        }
        reinterpret_cast<float4*>(dst)[c] = v;
    }
}
__device__ __forceinline__ void wide_row_out(float* __restrict__ dst, const float* __restrict__ src, int N, int nch, int tid) {
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    for (int c = tid; c < nch; c += WIDE_THREADS) {
        const float4 v = reinterpret_cast<const float4*>(src)[c];
        if (vec) reinterpret_cast<float4*>(dst)[c] = v;
        else {
            const int i = 4 * c;
            dst[i] = v.x; if (i + 1 < N) dst[i + 1] = v.y; if (i + 2 < N) dst[i + 2] = v.z; if (i + 3 < N) dst[i + 3] = v.w;
        }
    }
}

// One launch = one evaluation of every running problem (init = 0), or the start of a run (init = 1 fresh, 2 resumed).
// One workgroup per problem; a finished problem's workgroup leaves at once.  Wavefront 0 runs the state machine on the scalar
// state in LDS and posts the vector work; all 16 wavefronts do it.
__global__ __launch_bounds__(WIDE_THREADS)
void k_opt_wide_tick(const WideDev D, int init, int step_mode, const float* __restrict__ x0, const float* __restrict__ loss,
                     const float* __restrict__ grad, float* __restrict__ x_trial) {
    __shared__ double s_part[2 * WIDE_WAVES];
    __shared__ WCmd s_cmd[2];
    __shared__ OptScal s_state;
    __shared__ float s_al[SFX_HIST_MAX];
    __shared__ float s_ro[WIDE_RO];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!init && D.status[b] > 0) return;      // finished (1: run_fitting returned; 1000: LBFGS.step returned): left alone
    const int N = D.cfg.N, nch = D.Np / 4, slots = wide_ring_slots(D.cfg.hist_cap);
    float* rows = D.rows + (size_t)b * W_NROWS * D.Np;
    WgWork w{(unsigned)nch, (unsigned)tid, s_part};
    wide_row_in(rows + (size_t)(init ? W_X : W_GIN) * D.Np, (init ? x0 : grad) + (size_t)b * N, N, nch, tid);
    if (tid < 64) {
        WgLayer v{w, s_cmd, &s_state, s_al, s_ro, rows, D.hist + (size_t)b * 2 * slots * D.Np, (size_t)D.Np, slots, b,
                  D.trace, D.trace_n, D.trace_cap};
        WideState& st = D.st[b];
        float* ro_g = D.ro + (size_t)b * WIDE_RO;
        int status;
        if (init) {
            wide_begin(v, st, init);
            WIDE_WSYNC();
            status = init == 1 ? (int)WIDE_RUNNING : D.st[b].status;
        } else {
            for (int i = tid; i < slots; i += 64) s_ro[i] = ro_g[i];
            WIDE_WSYNC();
            status = wide_tick(v, D.cfg, st, step_mode, loss[b]);
            WIDE_WSYNC();
            for (int i = tid; i < slots; i += 64) ro_g[i] = s_ro[i];
        }
        v.stop();
        if (tid == 0) D.status[b] = status;
    } else {
        w.serve(s_cmd);
    }
    // (every thread wrote its own chunks of the trial point)
    wide_row_out(x_trial + (size_t)b * N, rows + (size_t)W_XT * D.Np, N, nch, tid);
}

// rows W_X / W_GIN of every problem -> the caller's packed [B][N]
__global__ __launch_bounds__(WIDE_THREADS)
void k_opt_wide_gather(const WideDev D, int which, float* __restrict__ out) {
    const int b = blockIdx.x;
    wide_row_out(out + (size_t)b * D.cfg.N, D.rows + ((size_t)b * W_NROWS + which) * D.Np, D.cfg.N, D.Np / 4, threadIdx.x);
}

struct sfx_opt_wide {
    DevAlloc mem;
    OptTrace trace;             // (D.trace / D.trace_n / D.trace_cap are its view)
    WideDev D{};
    int mode = -1;              // of the last sfx_opt_wide_begin (-1: none yet)
    int* status_host = nullptr; // pinned: the readback of sfx_opt_wide_active
    ~sfx_opt_wide() { if (status_host) (void)hipHostFree(status_host); }
};

extern "C" int sfx_opt_wide_create(const sfx_opt_wide_cfg* c, sfx_opt_wide** out) {
    if (!c || !out) { sfx_set_error("null argument"); return -1; }
    *out = nullptr;
    if (const int rc = opt_check_cfg("sfx_opt_wide_create", c, SFX_WIDE_NMAX, SFX_WIDE_MAX_GROUPS)) return rc;
    // every argument is accepted: from here on only the device can refuse, and ~sfx_opt_wide releases whatever was acquired by then
    std::unique_ptr<sfx_opt_wide> h(new sfx_opt_wide());
    WideDev& D = h->D;
    WideCfg& C = D.cfg;
    const int B = c->B, N = c->N;
    D.B = B; D.Np = (N + 3) & ~3;
    C.N = N;
    C.maxiters = c->maxiters; C.ftol = c->ftol; C.gtol = c->gtol; C.lr = c->lr;
    const OptDefaults d = opt_defaults(c);
    C.max_iter = d.max_iter; C.max_eval = d.max_eval;
    C.tol_grad = d.tol_grad; C.tol_change = d.tol_change;
    C.hist_cap = d.hist_cap;
    C.reuse = d.reuse;
    C.ngroups = c->n_groups > 0 ? c->n_groups : 1;
    std::vector<int> g_off(C.ngroups), g_len(C.ngroups);
    for (int i = 0, o = 0; i < C.ngroups; ++i) { g_len[i] = c->n_groups > 0 ? c->group_len[i] : N; g_off[i] = o; o += g_len[i]; }
    C.g_off = h->mem.up(g_off);
    C.g_len = h->mem.up(g_len);
    const size_t slots = (size_t)wide_ring_slots(C.hist_cap);
    D.rows = h->mem.zeros<float>((size_t)B * W_NROWS * D.Np);
    D.hist = h->mem.zeros<float>((size_t)B * 2 * slots * D.Np);
    D.ro = h->mem.zeros<float>((size_t)B * WIDE_RO);
    D.st = h->mem.zeros<WideState>(B);
    D.status = h->mem.zeros<int>(B);
    if (h->mem.failed) {
        sfx_set_error("sfx_opt_wide_create: device memory for %d problems of %d variables: %s", B, N, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    if (hipHostMalloc((void**)&h->status_host, (size_t)B * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError(); h->status_host = nullptr;
        sfx_set_error("sfx_opt_wide_create: pinned host memory for %d problems", B); return -2;
    }
    *out = h.release();
    return 0;
}

extern "C" void sfx_opt_wide_destroy(sfx_opt_wide* h) { delete h; }

extern "C" int sfx_opt_wide_begin(sfx_opt_wide* h, int32_t mode, int32_t resume, const float* x0_dev, float* x_trial_dev, void* stream) {
    if (const int rc = opt_check_begin("sfx_opt_wide_begin", !h || !x0_dev || !x_trial_dev, mode, resume, h ? h->mode : -1)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const WideDev& D = h->D;
    // (the ring needs no clearing: a recursion reads the hist_n rows written since the fresh start, and no others)
    if (!resume) { if (const int rc = h->trace.empty(D.B, s)) return rc; }
    h->mode = mode;
    hipLaunchKernelGGL(k_opt_wide_tick, dim3(D.B), dim3(WIDE_THREADS), 0, s, D, resume ? 2 : 1, mode, x0_dev,
                       (const float*)nullptr, (const float*)nullptr, x_trial_dev);
    SFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sfx_opt_wide_tell(sfx_opt_wide* h, const float* loss_dev, const float* grad_dev, float* x_trial_dev, void* stream) {
    if (const int rc = opt_check_tell("sfx_opt_wide_tell", "sfx_opt_wide_begin", !h || !loss_dev || !grad_dev || !x_trial_dev, h ? h->mode : -1)) return rc;
    const WideDev& D = h->D;
    hipLaunchKernelGGL(k_opt_wide_tick, dim3(D.B), dim3(WIDE_THREADS), 0, (hipStream_t)stream, D, 0, h->mode,
                       (const float*)nullptr, loss_dev, grad_dev, x_trial_dev);
    SFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sfx_opt_wide_active(sfx_opt_wide* h, int32_t* n_active_host, void* stream) {
    if (!h || !n_active_host) { sfx_set_error("sfx_opt_wide_active: null argument"); return -1; }
    if (h->mode < 0) { *n_active_host = 0; return 0; }
    hipStream_t s = (hipStream_t)stream;
    SFX_CHECK(hipMemcpyAsync(h->status_host, h->D.status, (size_t)h->D.B * sizeof(int), hipMemcpyDeviceToHost, s));
    SFX_CHECK(hipStreamSynchronize(s));
    int n = 0;
    for (int i = 0; i < h->D.B; ++i) n += h->status_host[i] == WIDE_RUNNING;
    *n_active_host = n;
    return 0;
}

extern "C" int sfx_opt_wide_get(sfx_opt_wide* h, float* x_dev, float* grad_dev, float* result_host, int32_t* evals_host, int32_t* status_host) {
    if (!h) { sfx_set_error("sfx_opt_wide_get: null handle"); return -1; }
    const WideDev& D = h->D;
    SFX_CHECK(hipDeviceSynchronize());
    if (x_dev) hipLaunchKernelGGL(k_opt_wide_gather, dim3(D.B), dim3(WIDE_THREADS), 0, (hipStream_t)0, D, (int)W_X, x_dev);
    if (grad_dev) hipLaunchKernelGGL(k_opt_wide_gather, dim3(D.B), dim3(WIDE_THREADS), 0, (hipStream_t)0, D, (int)W_GIN, grad_dev);
    SFX_CHECK(hipGetLastError());
    std::vector<WideState> st(D.B);
    SFX_CHECK(hipMemcpy(st.data(), D.st, st.size() * sizeof(WideState), hipMemcpyDeviceToHost));
    SFX_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < D.B; ++i) {
        if (result_host) result_host[i] = st[i].result;
        if (evals_host) evals_host[i] = st[i].evals;
        if (status_host) status_host[i] = (h->mode >= 0 && st[i].status > 0) ? 1 : 0;
    }
    return 0;
}

extern "C" int sfx_opt_wide_trace(sfx_opt_wide* h, int32_t capacity) {
    if (!h || capacity < 0) { sfx_set_error("sfx_opt_wide_trace: bad argument"); return -1; }
    const int rc = h->trace.attach("sfx_opt_wide_trace", h->D.B, capacity);
    h->trace.view(h->D.trace, h->D.trace_n, h->D.trace_cap);
    return rc;
}

extern "C" int sfx_opt_wide_get_trace(sfx_opt_wide* h, float* records, int32_t* counts) {
    return OptTrace::read(h ? &h->trace : nullptr, "sfx_opt_wide_trace", h ? h->D.B : 0, records, counts);
}
