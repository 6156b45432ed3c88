// gemm_small.hip -- NT GEMM for the LATENCY-CLASS 16-bit products: the SASRec user encoder's Linear layers over B S = 2 560 rows
// (T/model/modules.py:41-44,8-9: w_Q / w_K / w_V / fc, w_1 / w_2 at d_model = 512) and the products of the same size around them.
// On 128 x 128 tiles such a product is 80 - 320 workgroups whose two-buffer main loop exposes one global-load latency per 64-wide K
// stage: 10 - 33 us per launch at 60 - 170 TFLOP/s (profiles/r06_id_tower_step_before.txt).  Here: 64 x 64 tiles (four waves of 32 x 32),
// a four-stage LDS-DMA ring with counted waits (gemm_core.hpp, gemm_mainloop_ring), 64 KiB of LDS so that two workgroups share a CU.
// The epilogues are the generic kernel's (gemm_nt_generic.hpp): bias, ReLU / GELU (+ act'), x act' + column sums.  Outputs are
// bit-identical to the 128 x 128 kernel's: the same MFMA, the same K order per output element.
#include "gemm_nt_generic.hpp"

static_assert(GemmTileCfg<bf16, 2, 2, 2, 2, 2, 4>::TM == gplan::SMALL_T && GemmTileCfg<bf16, 2, 2, 2, 2, 2, 4>::TN == gplan::SMALL_T, "gemm_plan.hpp");

int gemm_small_launch(const GemmPlan& p, GemmArgs& a, hipStream_t s) {
    if (p.in_dtype == MOREC_F16) return launch_gemm_cfg<GemmTileCfg<f16, 2, 2, 2, 2, 2, 4>, f16, f16>(p, a, s);
    return launch_gemm_cfg<GemmTileCfg<bf16, 2, 2, 2, 2, 2, 4>, bf16, bf16>(p, a, s);
}
