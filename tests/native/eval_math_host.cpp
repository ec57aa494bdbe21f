// Test harness: compiles the filter-parameterised resample arithmetic of esvit_amd/csrc/augment_math.h for the HOST so that
// tests/test_eval_transform_cpu.py can check it against the numpy restatement without a GPU.  Not part of the library.
#define AUG_HD static inline
#include "augment_math.h"

extern "C" {
int eval_t_ksize(int filter, int in_size, int out_size) { return aug::resample_ksize_f(filter, in_size, out_size); }
// taps of output positions [lo, lo + n) of an axis resized in_size -> out_size
void eval_t_coeffs(int filter, int in_size, int out_size, int lo, int n, int kmax, int32_t* bounds, int32_t* kk) {
    for (int t = 0; t < n; ++t) {
        for (int i = 0; i < kmax; ++i) kk[t * kmax + i] = 0;
        aug::resample_row_f(filter, in_size, out_size, lo + t, kmax, bounds + 2 * t, bounds + 2 * t + 1, kk + t * kmax);
    }
}
}
