// pulse_body.inc -- the bodies of the pulse-shaping kernels (fir.hip), included textually INSIDE each kernel so that
// the Complex<f32> kernels (pulse_kernel, pulse_poly_kernel) and their input-view twins (pulse_in_kernel,
// pulse_poly_in_kernel: packed bits, comms_pulse_set_input_format) compile from the same tokens.  The c32
// kernels' code objects are exactly those of the bodies they had before the views existed (a shared
// __device__ function changed their scheduling and, at SPS 32, made one copy the argument block).
//   PULSE_GENERIC_BODY: pulse_kernel's parameters in scope; PULSE_SYM is the symbol input.
//   otherwise:          pulse_poly_kernel's (a, SPS, REAL, MIX); PULSE_SYM is the symbol input.
#ifdef PULSE_GENERIC_BODY
    extern __shared__ __attribute__((aligned(16))) char smem[];
    hist_advance(hist, PULSE_SYM, n_sym, new_hist, hist_len);
    float2* tp = reinterpret_cast<float2*>(smem);
    for (int k = threadIdx.x; k < n_taps; k += 256) tp[k] = taps[k];
    __syncthreads();
    const size_t n_out = n_sym * static_cast<size_t>(sps);
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    double rc = 1.0, rs = 0.0;
    if (mx.on) pulse_rotor_at(mx.turns0 + (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) * mx.frac, rc, rs);
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_out;
         i += stride) {
        const size_t m = i / sps;
        const int p = static_cast<int>(i - m * sps);
        float2 acc = make_float2(0.f, 0.f);
        long long s = static_cast<long long>(m);
        for (int k = p; k < n_taps; k += sps, --s) {
            const float2 x = stream_at(PULSE_SYM, hist, hist_len, s, n_sym);
            const float2 h = tp[k];
            acc.x = __builtin_fmaf(h.x, x.x, acc.x);
            acc.x = __builtin_fmaf(-h.y, x.y, acc.x);
            acc.y = __builtin_fmaf(h.x, x.y, acc.y);
            acc.y = __builtin_fmaf(h.y, x.x, acc.y);
        }
        if (mx.on) {  // Mixer::mix arithmetic: f64 product rounded once (src/mixer.rs:77-78)
            const double yr = acc.x, yi = acc.y;
            acc = make_float2(static_cast<float>(yr * rc - yi * rs), static_cast<float>(yr * rs + yi * rc));
            const double nc = rc * mx.sweep_c - rs * mx.sweep_s;
            rs = rc * mx.sweep_s + rs * mx.sweep_c;
            rc = nc;
        }
        if (mx.out_i16)
            reinterpret_cast<short2*>(out)[i] = c32_as_i16(acc, mx.out_scale);
        else
            out[i] = acc;
    }
#else
    constexpr int SPSP = SPS + (SPS & 1);
    // outputs leave through a per-wave LDS block, CW phases at a time (CW * 2 KiB per workgroup)
    constexpr int CW = SPS <= 8 ? SPS : SPS % 8 == 0 ? 8 : SPS % 6 == 0 ? 6 : SPS % 5 == 0 ? 5 : SPS % 4 == 0 ? 4 : SPS % 3 == 0 ? 3 : SPS % 2 == 0 ? 2 : 1;
    __shared__ cf sh[256 + PP_JMAX];
    __shared__ __attribute__((aligned(16))) cf xch[256 * CW];
    const int tid = threadIdx.x;
    const int halo = a.J - 1;
    const size_t ntiles = (a.n_sym + 255) / 256;
    kstamp_begin(a.ks);
    hist_advance(a.hist, PULSE_SYM, a.n_sym, a.new_hist, a.hist_len);
    double rc = 1.0, rs = 0.0;  // rotor of this lane's first output of the current tile
    if (MIX) pulse_rotor_at(a.mx.turns0 + (static_cast<uint64_t>(blockIdx.x) * 256 + tid) * SPS * a.mx.frac, rc, rs);
    // the next tile's symbols are requested before this tile's taps run and land in LDS at the top of the next step: a
    // tile's own work is short, and without this every step began with an exposed round trip to HBM
    cf nx0 = cf{0.f, 0.f}, nx1 = cf{0.f, 0.f};  // window elements tid and 256 + tid (the latter: tid < halo <= 127)
    auto fetch = [&](size_t t) {
        const long long w0 = static_cast<long long>(t) * 256 - halo;
        nx0 = to_cf(stream_at(PULSE_SYM, a.hist, a.hist_len, w0 + tid, a.n_sym));
        if (tid < halo) nx1 = to_cf(stream_at(PULSE_SYM, a.hist, a.hist_len, w0 + 256 + tid, a.n_sym));
    };
    if (blockIdx.x < ntiles) fetch(blockIdx.x);
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long m0 = static_cast<long long>(t) * 256;
        __syncthreads();
        sh[tid] = nx0;
        if (tid < halo) sh[256 + tid] = nx1;
        __syncthreads();
        if (t + gridDim.x < ntiles) fetch(t + gridDim.x);
        cf acc[SPS];
#pragma unroll
        for (int p = 0; p < SPS; ++p) acc[p] = cf{0.f, 0.f};
        const cf* sp = sh + halo + tid;
        for (int j0 = 0; j0 < a.J; j0 += PP_JB) {
            cf sv[PP_JB];
            v2f tr[PP_JB * SPSP / 2], ti[PP_JB * SPSP / 2];
#pragma unroll
            for (int i = 0; i < PP_JB * SPSP / 2; ++i) {
                tr[i] = v2f{a.are[j0 * SPSP + 2 * i], a.are[j0 * SPSP + 2 * i + 1]};
                if (!REAL) ti[i] = v2f{a.aim[j0 * SPSP + 2 * i], a.aim[j0 * SPSP + 2 * i + 1]};
            }
#pragma unroll
            for (int jj = 0; jj < PP_JB; ++jj) sv[jj] = sp[-(j0 + jj)];
#pragma unroll
            for (int jj = 0; jj < PP_JB; ++jj)
#pragma unroll
                for (int p = 0; p < SPS; ++p) {
                    const int e = jj * SPSP + p;
                    mac_tap<REAL>(acc[p], sv[jj], tr[e >> 1], ti[e >> 1], (e & 1) != 0);
                }
        }
        if (MIX) {
            const cf r0 = cf{static_cast<float>(rc), static_cast<float>(rs)};
#pragma unroll
            for (int p = 0; p < SPS; ++p) acc[p] = cmulf(acc[p], p ? cmulf(r0, to_cf(a.step[p])) : r0);
            const double nc = rc * a.mx.sweep_c - rs * a.mx.sweep_s;
            rs = rc * a.mx.sweep_s + rs * a.mx.sweep_c;
            rc = nc;
        }
        {
            // A lane's SPS outputs are one run of SPS * 8 B, so a plain store instruction covers a wave's 64 SPS outputs in
            // pieces of 16 B at a stride of SPS * 8 B.  Through the wave's own LDS block instead, CW <= 8 phases at a time:
            // instruction i writes elements 64 i ... 64 i + 63 of the block [64 symbols][CW], i.e. whole lines for SPS <= 8
            // and runs of CW * 8 B above (63 taps x 4, 2^26 outputs: 183 -> 134 us; 127 taps x 8, 2^24: 48.8 -> 29.7 us).
            cf* ex = xch + (tid & ~63) * CW;
            const int lane = tid & 63;
            const size_t mw = static_cast<size_t>(m0) + (tid & ~63);                      // the wave's first symbol
            const unsigned nel = mw < a.n_sym ? static_cast<unsigned>(a.n_sym - mw < 64 ? a.n_sym - mw : 64) * CW : 0u;  // valid elements per chunk
#pragma unroll
            for (int c = 0; c < SPS / CW; ++c) {
                if (c) {  // the previous chunk has been read
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
#pragma unroll
                for (int p = 0; p < CW; ++p) ex[lane * CW + p] = acc[c * CW + p];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (a.mx.out_i16) {  // the transmit chain straight into the IQOutput wire format: 4 B per output
                    constexpr int W = CW % 4 == 0 ? 4 : CW % 2 == 0 ? 2 : 1;  // outputs per lane and store
                    short2* o = reinterpret_cast<short2*>(a.out) + mw * SPS + c * CW;
#pragma unroll
                    for (int i = 0; i < CW / W; ++i) {
                        const unsigned e = (static_cast<unsigned>(i) * 64u + lane) * W;
                        if (e < nel) {  // (nel is a multiple of CW, hence of W)
                            short2 q[W];
#pragma unroll
                            for (int w = 0; w < W; ++w) q[w] = c32_as_i16(to_f2(ex[e + w]), a.mx.out_scale);
                            short2* dp = o + (e / CW) * SPS + e % CW;
                            if constexpr (W == 4) {
                                u32x4 qv;
                                __builtin_memcpy(&qv, q, 16);
                                store_b128_dword_aligned(dp, qv);
                            } else if constexpr (W == 2) {
                                __builtin_memcpy(dp, q, 8);
                            } else {
                                dp[0] = q[0];
                            }
                        }
                    }
                } else {
                    constexpr int W = CW % 2 == 0 ? 2 : 1;
                    float2* o = a.out + mw * SPS + c * CW;
#pragma unroll
                    for (int i = 0; i < CW / W; ++i) {
                        const unsigned e = (static_cast<unsigned>(i) * 64u + lane) * W;
                        if (e < nel) {
                            float2* dp = o + (e / CW) * SPS + e % CW;
                            if constexpr (W == 2) {
                                const cf u0 = ex[e], u1 = ex[e + 1];
                                float2 q[2] = {to_f2(u0), to_f2(u1)};
                                __builtin_memcpy(dp, q, 16);
                            } else {
                                dp[0] = to_f2(ex[e]);
                            }
                        }
                    }
                }
            }
        }
    }
    kstamp_end(a.ks);
#endif
