// input_expand.hip -- the library's copy of the expand kernels of a compact upload (input_expand.h has them and says what they do).
#include "ald_internal.h"
#include "input_expand.h"

int ald_expand_input(const ald_batch *b, hipStream_t st)
{
    const unsigned derive = derive_mask(b->sec);
    if(!derive) return ALD_OK;
    const BatchIn in = b->hb.make_batch_in((uint8_t*)b->d_in.p, b->sec);
    const hipError_t e = expand_input(in, (const int32_t*)b->d_gsid.p, b->hb.off_v.back(), b->hb.off_e.back(), derive, st);
    return e == hipSuccess ? ALD_OK : ald_set_err(ALD_ERR_HIP, std::string("expand kernels of the compact upload: ") + hipGetErrorString(e));
}
