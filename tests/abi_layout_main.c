/* The layout a C compiler gives the structs of include/cloudaae_hip.h: size, then the offset of every field, one per line
 * (tests/test_capi_symbols.py compiles and runs this and compares with the ctypes classes of cloudaae_amd/_lib.py). */
#include "cloudaae_hip.h"

#include <stddef.h>
#include <stdio.h>

#define S(T) printf(#T " sizeof %zu\n", sizeof(T))
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
#define JOB(f) F(cloudaae_gemm_tn_job, f)
#define SYNC(f) F(cloudaae_bn_sync, f)
#define FC(f) F(cloudaae_fc_layer, f)

int main(void)
{
    S(cloudaae_gemm_tn_job);
    JOB(M); JOB(N); JOB(K); JOB(A); JOB(lda); JOB(B); JOB(ldb); JOB(C); JOB(ldc); JOB(fold_c); JOB(zeroed);
    S(cloudaae_bn_sync);
    SYNC(allreduce); SYNC(ctx); SYNC(world); SYNC(buf);
    S(cloudaae_fc_layer);
    FC(K); FC(N); FC(x); FC(ldx); FC(w); FC(bias); FC(gamma); FC(beta); FC(ema_mean); FC(ema_var); FC(save_mean);
    FC(save_var); FC(relu); FC(y); FC(out); FC(tickets); FC(dout); FC(lddo); FC(dx); FC(lddx); FC(dw); FC(accumulate_dw);
    FC(dgamma); FC(dbeta); FC(dbias); FC(accumulate_param_grads); FC(partials); FC(partials_floats); FC(out_rowvec);
    FC(out_rowvec_d);
    return 0;
}
