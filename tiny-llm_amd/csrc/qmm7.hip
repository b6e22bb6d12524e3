// Launcher of the row-streaming batched-decode matmul (qmm7.h).
#include "qmm7.h"

namespace tl {

// the dispatch is generated from the instantiation table (linear_plan.h, QM7_TABLE)
#ifndef QM7_LAB_NB
#define QM7_LAB_NB 0
#endif
#ifndef QM7_LAB_OCC
#define QM7_LAB_OCC 1
#endif
template <int MB, int T, int GPW, int EPI>
static int launch_one7(const Qmm6Args &a, const Qmm7Plan &pl, hipStream_t st) {
    auto kern = qmm7_kernel<MB, T, GPW, EPI, QM7_LAB_NB, QM7_LAB_OCC>;
    if (pl.lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    hipLaunchKernelGGL(kern, dim3(pl.wgs, pl.row_blocks), dim3(QM7_WAVES * 64), pl.lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <int T, int GPW, int EPI>
static int launch_rows7(const Qmm6Args &a, const Qmm7Plan &pl, hipStream_t st) {
    switch (pl.MB) {
        case 1: return launch_one7<1, T, GPW, EPI>(a, pl, st);
        case 2: return launch_one7<2, T, GPW, EPI>(a, pl, st);
        case 3: return launch_one7<3, T, GPW, EPI>(a, pl, st);
        case 4: return launch_one7<4, T, GPW, EPI>(a, pl, st);
    }
    return -2;
}
template <int EPI>
static int launch_variant7(const Qmm6Args &a, const Qmm7Plan &pl, hipStream_t st) {
#define QM7_CASE(Tv, GPWv) \
    if (pl.T == Tv && pl.GPW == GPWv) return launch_rows7<Tv, GPWv, EPI>(a, pl, st);
    QM7_TABLE(QM7_CASE)
#undef QM7_CASE
    return -2;
}

int launch_qmm7_bf16(const Qmm6Args &args, const Qmm7Plan &pl, int epi, hipStream_t st) {
    if (!args.a_frag || !args.ss) return -1;  // weighted rows in fragment order, with their sums of squares
    if (args.ss_n <= 0 || args.ss_n > QM6_SS_MAX || args.ss_n % 4 != 0) return -1;
    if (args.out_w || args.ss_out || args.residual) return -1;
    if (!pl.ok) return -1;
    if (epi == EPI_STORE) return launch_variant7<EPI_STORE>(args, pl, st);
    if (epi == EPI_SWIGLU) return launch_variant7<EPI_SWIGLU>(args, pl, st);
    return -1;
}

}  // namespace tl
