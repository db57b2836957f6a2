/*
 * ORACLE (test infrastructure, NOT product code): plain-C/OpenMP restatement of the three hot-path
 * stencils with the structure of gt4py's `gt:cpu_ifirst` backend -- I-contiguous fields
 * (layout (2,1,0), /root/reference/src/gt4py/storage/cartesian/layout_registry.py:87-94), threads
 * over (K, J) rows, I innermost; K innermost and serial for the vertical solve.
 *
 * Used (a) as a second, independent check of the numpy restatement (tests/test_oracle.py), (b) as the CPU baseline timed
 * next to the GPU numbers (bench.py "cpu_baseline", kind "port", oracle_lap5_f64 only) and (c) as the whole-field oracle of
 * the full-size GPU tests (tests/fullsize_util.py): every variant, dtype and internal precision the kernel library ships.
 * It is NOT GridTools: the reference's gt:cpu_ifirst needs gridtools-cpp 2.3.9 headers that are not
 * in this image.  Same arithmetic as oracle/ref_numpy.py: expression trees
 * of the stencil definitions, one rounding per operation; build with -ffp-contract=off.
 *
 * Definitions restated: examples/lap_cartesian_vs_next.ipynb cell 7;
 * tests/cartesian_tests/integration_tests/multi_feature_tests/stencil_definitions.py:316-328, :219-232
 * (all under /root/reference).
 *
 * Fields are described by an origin-shifted pointer and element strides (si, sj, sk).
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifdef _OPENMP
#include <omp.h>
#endif

#pragma STDC FP_CONTRACT OFF

void oracle_set_threads(int n) {
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

int oracle_max_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* out = -4.0*in + in[-1,0] + in[1,0] + in[0,-1] + in[0,1]   (left-associative) */
void oracle_lap5_f64(const double* in, int64_t isi, int64_t isj, int64_t isk, double* out, int64_t osi,
                     int64_t osj, int64_t osk, int64_t di, int64_t dj, int64_t dk) {
#pragma omp parallel for collapse(2) schedule(static)
    for (int64_t k = 0; k < dk; ++k)
        for (int64_t j = 0; j < dj; ++j) {
            const double* p = in + k * isk + j * isj;
            double* q = out + k * osk + j * osj;
            for (int64_t i = 0; i < di; ++i) {
                const double* c = p + i * isi;
                double r = -4.0 * c[0];
                r = r + c[-isi];
                r = r + c[isi];
                r = r + c[-isj];
                r = r + c[isj];
                q[i * osi] = r;
            }
        }
}

/* All four Laplacian variants of csrc/lap5.hip.h:lap5_expr (GT4MI_LAP_NOTEBOOK / DOCS / SUITE / AVG = 0 / 1 / 2 / 3).
 * T = field type, W = dtype the float literals promote to (double by default; float for float fields under
 * literal_float_precision=32).  Each bracket sum is evaluated in T, every other operation in W, one rounding to T at the end.
 * c = in[0,0], w = in[-1,0], e = in[+1,0], s = in[0,-1], n = in[0,+1]. */
#define LAP5_LOOP(T, EXPR)                                                                             \
    _Pragma("omp parallel for collapse(2) schedule(static)")                                           \
    for (int64_t k = 0; k < dk; ++k)                                                                   \
        for (int64_t j = 0; j < dj; ++j) {                                                             \
            const T* p = in + k * isk + j * isj;                                                       \
            T* q = out + k * osk + j * osj;                                                            \
            for (int64_t i = 0; i < di; ++i) {                                                         \
                const T* x = p + i * isi;                                                              \
                const T c = x[0], w = x[-isi], e = x[isi], s = x[-isj], n = x[isj];                    \
                (void)c; /* (the avg variant does not read the centre) */                              \
                q[i * osi] = (EXPR);                                                                   \
            }                                                                                          \
        }

#define LAP5_IMPL(NAME, T, W)                                                                          \
    int NAME(const T* in, int64_t isi, int64_t isj, int64_t isk, T* out, int64_t osi, int64_t osj,     \
             int64_t osk, int64_t di, int64_t dj, int64_t dk, int variant) {                           \
        if (variant == 0) {                                                                            \
            LAP5_LOOP(T, (T)(((((((W)(-4.0) * (W)c) + (W)w) + (W)e) + (W)s) + (W)n)))                  \
        } else if (variant == 1) {                                                                     \
            LAP5_LOOP(T, (T)(((W)(-4.0) * (W)c) + (W)(T)(((e + w) + n) + s)))                          \
        } else if (variant == 2) {                                                                     \
            LAP5_LOOP(T, (T)(((W)4.0 * (W)c) - (W)(T)(((e + w) + n) + s)))                             \
        } else if (variant == 3) {                                                                     \
            LAP5_LOOP(T, (T)((W)0.25 * (W)(T)(((n + s) + e) + w)))                                     \
        } else {                                                                                       \
            return -1;                                                                                 \
        }                                                                                              \
        return 0;                                                                                      \
    }

LAP5_IMPL(oracle_lap5_f64_variant, double, double)
LAP5_IMPL(oracle_lap5_f32, float, double)
LAP5_IMPL(oracle_lap5_f32_lit32, float, float)

/* Horizontal diffusion, optional flux limiter, in the (W, PW) combinations csrc/hdiff.hip.h:hdiff_run dispatches to.
 * T = field type, W = dtype of lap / flx / fly, PW = dtype of coeff * (...) and of the final subtraction.  The coefficient
 * is the field `cf` or, when `cf` is NULL, the scalar `coeff` rounded to PW.
 * Row-blocked: per (k, j) the lap rows it needs are recomputed into small heap buffers, which is value-identical to full
 * temporaries. */
#define HDIFF_IMPL(NAME, T, W, PW)                                                                   \
    void NAME(const T* in, int64_t isi, int64_t isj, int64_t isk, T* out, int64_t osi, int64_t osj,   \
              int64_t osk, const T* cf, int64_t csi, int64_t csj, int64_t csk, double coeff,         \
              int64_t di, int64_t dj, int64_t dk, int limiter) {                                     \
        _Pragma("omp parallel") {                                                                    \
            W* lapm = (W*)malloc(sizeof(W) * (size_t)(di + 2) * 3);                                  \
            W* lap0 = lapm + (di + 2);                                                               \
            W* lapp = lap0 + (di + 2);                                                               \
            const PW cs = (PW)coeff;                                                                 \
            _Pragma("omp for collapse(2) schedule(static)")                                          \
            for (int64_t k = 0; k < dk; ++k)                                                         \
                for (int64_t j = 0; j < dj; ++j) {                                                   \
                    const T* base = in + k * isk + j * isj;                                          \
                    /* lap on rows j-1, j, j+1 for i in [-1, di] */                                  \
                    for (int r = -1; r <= 1; ++r) {                                                  \
                        W* dst = r < 0 ? lapm : (r == 0 ? lap0 : lapp);                              \
                        const T* row = base + r * isj;                                               \
                        for (int64_t i = -1; i <= di; ++i) {                                         \
                            const T* c = row + i * isi;                                              \
                            const T sum = ((c[isi] + c[-isi]) + c[isj]) + c[-isj];                   \
                            dst[i + 1] = ((W)4.0 * (W)c[0]) - (W)sum;                                \
                        }                                                                            \
                    }                                                                                \
                    for (int64_t i = 0; i < di; ++i) {                                               \
                        const T* c = base + i * isi;                                                 \
                        W flx, flxm, fly, flym, res;                                                 \
                        res = lap0[i + 2] - lap0[i + 1];                                             \
                        flx = (limiter && (res * (W)(T)(c[isi] - c[0])) > (W)0) ? (W)0 : res;        \
                        res = lap0[i + 1] - lap0[i];                                                 \
                        flxm = (limiter && (res * (W)(T)(c[0] - c[-isi])) > (W)0) ? (W)0 : res;      \
                        res = lapp[i + 1] - lap0[i + 1];                                             \
                        fly = (limiter && (res * (W)(T)(c[isj] - c[0])) > (W)0) ? (W)0 : res;        \
                        res = lap0[i + 1] - lapm[i + 1];                                             \
                        flym = (limiter && (res * (W)(T)(c[0] - c[-isj])) > (W)0) ? (W)0 : res;      \
                        const W s = ((flx - flxm) + fly) - flym;                                     \
                        const PW cv = cf ? (PW)cf[k * csk + j * csj + i * csi] : cs;                 \
                        out[k * osk + j * osj + i * osi] = (T)((PW)c[0] - (cv * (PW)s));             \
                    }                                                                                \
                }                                                                                    \
            free(lapm);                                                                              \
        }                                                                                            \
    }

HDIFF_IMPL(oracle_hdiff_f64, double, double, double)
HDIFF_IMPL(oracle_hdiff_f32, float, double, double)
HDIFF_IMPL(oracle_hdiff_f32_w32, float, float, float)
HDIFF_IMPL(oracle_hdiff_f32_w32_p64, float, float, double)

/* Thomas solve, column by column (K innermost, serial); threads over (J, I-blocks).  T = field type, arithmetic in T. */
#define TRIDIAG_IMPL(NAME, T)                                                                          \
    void NAME(const T* inf, const T* diag, T* sup, T* rhs, T* out,                                     \
              int64_t si, int64_t sj, int64_t sk, int64_t di, int64_t dj, int64_t dk) {                \
    _Pragma("omp parallel for schedule(static)")                                                       \
        for (int64_t j = 0; j < dj; ++j) {                                                             \
            /* level by level over a whole row of columns keeps the I-contiguous accesses streaming */ \
            const int64_t r = j * sj;                                                                  \
            for (int64_t i = 0; i < di; ++i) {                                                         \
                const int64_t o = r + i * si;                                                          \
                sup[o] = sup[o] / diag[o];                                                             \
                rhs[o] = rhs[o] / diag[o];                                                             \
            }                                                                                          \
            for (int64_t k = 1; k < dk; ++k) {                                                         \
                const int64_t b = r + k * sk;                                                          \
                for (int64_t i = 0; i < di; ++i) {                                                     \
                    const int64_t o = b + i * si, m = o - sk;                                          \
                    const T den1 = diag[o] - (sup[m] * inf[o]);                                        \
                    const T ns = sup[o] / den1;                                                        \
                    const T num = rhs[o] - (inf[o] * rhs[m]);                                          \
                    const T den2 = diag[o] - (sup[m] * inf[o]);                                        \
                    sup[o] = ns;                                                                       \
                    rhs[o] = num / den2;                                                               \
                }                                                                                      \
            }                                                                                          \
            {                                                                                          \
                const int64_t b = r + (dk - 1) * sk;                                                   \
                for (int64_t i = 0; i < di; ++i) out[b + i * si] = rhs[b + i * si];                    \
            }                                                                                          \
            for (int64_t k = dk - 2; k >= 0; --k) {                                                    \
                const int64_t b = r + k * sk;                                                          \
                for (int64_t i = 0; i < di; ++i) {                                                     \
                    const int64_t o = b + i * si;                                                      \
                    out[o] = rhs[o] - (sup[o] * out[o + sk]);                                          \
                }                                                                                      \
            }                                                                                          \
        }                                                                                              \
    }

TRIDIAG_IMPL(oracle_tridiag_f64, double)
TRIDIAG_IMPL(oracle_tridiag_f32, float)
