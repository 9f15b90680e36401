// qs_sweep.inl - the sweep kernel of qstate.hip, included twice.  QS_SWEEP_MODES 0: qs_sweep_kernel<CLUSTER>, the two
// forms a handle without binner and without exchange rounds runs; their text is what it was before the modes existed, so
// that their device code stays what it was (tools/diff_kernel_isa.py).  QS_SWEEP_MODES 1: qs_sweep_kernel<CLUSTER, BIN,
// DEFER> with a BinArgs argument.  BIN: lane 0 pushes every measurement it takes into the walker's binner, right behind
// the sums and the series record.  DEFER: the launch's last sweep is followed by an exchange round and is measured; its
// measurement is left to qs_exchange_kernel.
//
// CLUSTER = false is the sweep without moves (ca is not read); CLUSTER = true runs the walker's cluster move behind the
// colour passes of every sweep whose global index is a multiple of ca.rate (> 0)
#if QS_SWEEP_MODES
template <bool CLUSTER, bool BIN, bool DEFER>
#else
template <bool CLUSTER>
#endif
__global__ __launch_bounds__(THREADS) void qs_sweep_kernel(DevState s, const int *__restrict__ site,
                                                           const int4 *__restrict__ rows, const int *__restrict__ off,
                                                           const long long *__restrict__ e_q30,
                                                           const int2 *__restrict__ cs_q30, int C, int n_sweeps,
                                                           long long first_sweep, long long thermalization,
#if QS_SWEEP_MODES
                                                           int measure_rate, ClusterArgs ca, BinArgs ba)
#else
                                                           int measure_rate, ClusterArgs ca)
#endif
{
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x, nt = blockDim.x, w = blockIdx.x;
    const int N = s.N, Nw = s.Nw, q = s.q, z = s.z;
    double *wt = (double *)lds;                                // [q][q]
    long long *et = (long long *)(wt + q * q);                 // [q]
    int2 *cs = (int2 *)(et + q);                               // [q]
    unsigned long long *red = (unsigned long long *)(cs + q);  // E_int, Mx, My, accepted sites of the launch
    unsigned char *st = (unsigned char *)(red + 4);            // [4 Nw]
    {
        unsigned int *stw = (unsigned int *)st;
        const unsigned int *src = s.conf + (size_t)w * Nw;
        for (int j = tid; j < Nw; j += nt) stw[j] = src[j];
        const double *wsrc = s.wt + (size_t)w * q * q;
        for (int j = tid; j < q * q; j += nt) wt[j] = wsrc[j];
        for (int j = tid; j < q; j += nt) {
            et[j] = e_q30[j];
            cs[j] = cs_q30[j];
        }
        if (tid == 0) {
            red[0] = (unsigned long long)s.E[w];
            red[1] = (unsigned long long)s.Mx[w];
            red[2] = (unsigned long long)s.My[w];
            red[3] = 0ull;
        }
    }
    const unsigned long long key = s.key[w];
    unsigned long long sc = s.cursor[w];
    // lane 0 carries the walker's sums through the launch
    double sE = 0.0, sE2 = 0.0, sM = 0.0, sM2 = 0.0, sM4 = 0.0;
    long long n_meas = 0, n_series = 0;
#if QS_SWEEP_MODES
    [[maybe_unused]] long long bin_T = ba.T;  // (BIN) the pushes the binner stands at, the same for every walker
#endif
    if (tid == 0) {
        sE = s.sE[w];
        sE2 = s.sE2[w];
        sM = s.sM[w];
        sM2 = s.sM2[w];
        sM4 = s.sM4[w];
        n_meas = s.n_meas[w];
        n_series = s.n_series[w];
    }
    // the next measured sweep at or behind first_sweep: one division per launch, none per sweep
    const long long g0 = first_sweep > thermalization + 1 ? first_sweep : thermalization + 1;
    long long next = (g0 + measure_rate - 1) / measure_rate * measure_rate;
    long long dE = 0, dMx = 0, dMy = 0;
    int acc = 0;
    const double qm1 = (double)(q - 1);
    // (CLUSTER) the move cursor in every lane, the next sweep with a move, and lane 0's global counters
    unsigned long long mc = 0ull;
    long long next_move = 0, g_prop = 0, g_acc = 0, g_size = 0;
    if constexpr (CLUSTER) {
        mc = ca.cursor[w];
        next_move = (first_sweep + ca.rate - 1) / ca.rate * ca.rate;
    }
    __syncthreads();

    for (int sw = 0; sw < n_sweeps; ++sw, ++sc) {
        const unsigned int c1 = (unsigned int)sc, c3 = (unsigned int)(sc >> 32);
        for (int c = 0; c < C; ++c) {
            const int e1 = off[c + 1];
            for (int e = off[c] + tid; e < e1; e += nt) {
                const int i = site[e];
                const int4 r0 = rows[2 * e], r1 = rows[2 * e + 1];
                const int row[MAX_Z] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                const int so = st[i];
                double u1, u2;
                philox4_two(key, (unsigned int)i, c1, DOMAIN_SWEEP, c3, u1, u2);
                int t = so + 1 + min(q - 2, (int)(u1 * qm1));
                t = t >= q ? t - q : t;
                long long d = 0;
                double p = 1.0;
#pragma unroll
                for (int k = 0; k < MAX_Z; ++k)
                    if (k < z) {
                        const int sj = st[row[k]];
                        const int a = mod_q(so - sj, q), b = mod_q(t - sj, q);
                        d += et[a] - et[b];
                        p = p * wt[a * q + b];
                    }
                if (d <= 0 || u2 < p) {
                    st[i] = (unsigned char)t;
                    const int2 co = cs[so], cn = cs[t];
                    dE += d;
                    dMx += (long long)cn.x - co.x;  // (up to 2^31 in magnitude: not an int)
                    dMy += (long long)cn.y - co.y;
                    ++acc;
                }
            }
            __syncthreads();
        }
        const long long g = first_sweep + sw;  // global 1-based sweep index
        if constexpr (CLUSTER) {
            if (g == next_move) {  // (uniform)
                next_move += ca.rate;
                const int size = qs_cluster_move_lds(st, wt, et, cs, (unsigned int *)(st + 4 * Nw), ca.nbr, N, q, z, key, mc,
                                                     dE, dMx, dMy);
                ++mc;
                g_prop += 1;
                g_acc += size > 1;
                g_size += size;
            }
        }
        if (g != next) continue;               // (uniform)
#if QS_SWEEP_MODES
        if constexpr (DEFER)
            if (sw == n_sweeps - 1) continue;  // (uniform) the exchange kernel measures this sweep behind its round
#endif
        next += measure_rate;
        const long long e = wave_sum(dE), mx = wave_sum(dMx), my = wave_sum(dMy);
        dE = dMx = dMy = 0;
        if ((tid & (WAVE - 1)) == 0) {
            atomicAdd(&red[0], (unsigned long long)e);
            atomicAdd(&red[1], (unsigned long long)mx);
            atomicAdd(&red[2], (unsigned long long)my);
        }
        __syncthreads();  // (the next write of red[0..2] lies behind the next sweep's barriers)
        if (tid == 0) {
            const long long E = (long long)red[0], Mx = (long long)red[1], My = (long long)red[2];
            const double ev = (double)E * Q30_INV, x = (double)Mx * Q30_INV, y = (double)My * Q30_INV;
            const double m2 = x * x + y * y;
            sE = sE + ev;
            sE2 = sE2 + ev * ev;
            sM2 = sM2 + m2;
            sM4 = sM4 + m2 * m2;
            sM = sM + sqrt(m2);
            n_meas += 1;
            if (n_series < s.cap) {
                long long *rec = s.ser + ((size_t)w * s.cap + (size_t)n_series) * 3;
                rec[0] = E;
                rec[1] = Mx;
                rec[2] = My;
                n_series += 1;
            }
#if QS_SWEEP_MODES
            if constexpr (BIN) {
                qs_bin_push(ba, s.W, w, bin_T, ev, sqrt(m2), m2, m2 * m2);
                bin_T += 1;
            }
#endif
        }
    }

    __syncthreads();
    {
        const long long e = wave_sum(dE), mx = wave_sum(dMx), my = wave_sum(dMy), n = wave_sum((long long)acc);
        if ((tid & (WAVE - 1)) == 0) {
            atomicAdd(&red[0], (unsigned long long)e);
            atomicAdd(&red[1], (unsigned long long)mx);
            atomicAdd(&red[2], (unsigned long long)my);
            atomicAdd(&red[3], (unsigned long long)n);
        }
    }
    __syncthreads();
    {
        const unsigned int *stw = (const unsigned int *)st;
        unsigned int *dst = s.conf + (size_t)w * Nw;
        for (int j = tid; j < Nw; j += nt) dst[j] = stw[j];
    }
    if (tid == 0) {
        const long long prop = s.prop[w], accd = s.acc[w];  // requested together
        s.E[w] = (long long)red[0];
        s.Mx[w] = (long long)red[1];
        s.My[w] = (long long)red[2];
        s.prop[w] = prop + (long long)n_sweeps * N;
        s.acc[w] = accd + (long long)red[3];
        s.cursor[w] = sc;
        s.sE[w] = sE;
        s.sE2[w] = sE2;
        s.sM[w] = sM;
        s.sM2[w] = sM2;
        s.sM4[w] = sM4;
        s.n_meas[w] = n_meas;
        s.n_series[w] = n_series;
        if constexpr (CLUSTER) {
            ca.prop[w] += g_prop;
            ca.acc[w] += g_acc;
            ca.sum_size[w] += g_size;
            ca.cursor[w] = mc;
        }
    }
}
