// Host functions that one translation unit defines and another calls.  The calling file includes this header, and so does the
// defining file among the matrix-core and GEMV sources (gemm_*_fp4.hip, gemm_*_nf4.hip, gemv_*.hip), so one declaration is read beside
// the definition and beside every call instead of a hand-written copy at the point of use.  The sweep hooks of the dequant and
// quantiser sources are declared here for capi.hip only; a file that defines one should include this header the next time it is edited.
#pragma once

#include "fp4_common.h"

namespace fp4 {

// gemm_small_nf4.hip, for the entry points of gemm_wide_nf4.hip (which validate): 1..16 rows, K % 512 == 0, any form.  Launch only.
struct Nf4Call;  // nf4_call.h
void gemm_small_nf4_launch(const Nf4Call &call);

// gemv_fp4.hip, for the plain NF4 GEMV's irregular shapes (gemv_nf4.hip): the generic kernel with `table` as its code
struct Fp4Call;  // fp4_call.h
int gemv_generic_table(const Fp4Call &call, int table);

// gemm_wide_fp4.hip, gemm_splitk_fp4.hip, for gemm_small_fp4.hip: FP4_OK after the launch, -1 where the shape is not theirs
int gemm_wide_launch(const Fp4Call &call, bool any_rows);
int gemm_splitk_launch(const Fp4Call &call);
int64_t gemm_splitk_workspace_bytes(int64_t B, int64_t M, int64_t K, int blocksize, int dtype);

// sweep hooks behind fp4_hip_set_variant (capi.hip), each defined beside the kernels it steers
void set_dequant_variant(int v);       // dequant_fp4.hip
void set_gemv_variant(int v);          // gemv_fp4.hip
void set_small_variant(int v);         // gemm_small_fp4.hip
void set_wide_variant(int v);          // gemm_wide_fp4.hip
void set_quantize_variant(int v);      // quantize_fp4.hip
void set_gemv_nf4_variant(int v);      // gemv_nf4.hip
void set_wide_nf4_variant(int v);      // gemm_wide_nf4.hip

}  // namespace fp4
