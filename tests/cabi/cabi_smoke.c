/* Plain-C consumer of include/sdt_hip.h: proves the boundary is a C ABI (no C++ / torch types in the signatures).
 * Runs without a GPU: only the argument-validation paths are exercised (they return before any launch). */
#include <stdio.h>
#include <string.h>

#include <stddef.h>

#include "sdt_hip.h"

/* The structures' layout as the header's fields intend it, checked where a C consumer compiles (C11: _Static_assert; C99: an array
 * type of negative size).  The counts are the header's field lists: tests/test_abi_contract_host.py holds the ctypes mirrors of
 * speechdrivestemplates_amd/_lib.py to the same numbers through the compiler. */
#if defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
#define SDT_STATIC_ASSERT(cond, name) _Static_assert(cond, #name)
#else
#define SDT_STATIC_ASSERT(cond, name) typedef char sdt_static_assert_##name[(cond) ? 1 : -1]
#endif
SDT_STATIC_ASSERT(SDT_ABI_VERSION == 5, abi_version);
SDT_STATIC_ASSERT(sizeof(int32_t) == 4 && sizeof(float) == 4 && sizeof(double) == 8 && sizeof(void*) == 8, lp64_scalars);
/* 17 int32_t scalars, then dy, dx, wt of SDT_MAX_TAPS int32_t each */
SDT_STATIC_ASSERT(sizeof(sdt_conv_geom) == (17 + 3 * SDT_MAX_TAPS) * sizeof(int32_t), conv_geom_size);
SDT_STATIC_ASSERT(offsetof(sdt_conv_geom, dy) == 17 * sizeof(int32_t), conv_geom_dy);
SDT_STATIC_ASSERT(offsetof(sdt_conv_geom, wt) == (17 + 2 * SDT_MAX_TAPS) * sizeof(int32_t), conv_geom_wt);
/* six pointers, float slope, int32_t groups */
SDT_STATIC_ASSERT(sizeof(sdt_norm_bwd) == 6 * sizeof(void*) + sizeof(float) + sizeof(int32_t), norm_bwd_size);
SDT_STATIC_ASSERT(offsetof(sdt_norm_bwd, slope) == 6 * sizeof(void*), norm_bwd_slope);
SDT_STATIC_ASSERT(offsetof(sdt_norm_bwd, groups) == 6 * sizeof(void*) + sizeof(float), norm_bwd_groups);
/* four pointers, six int32_t */
SDT_STATIC_ASSERT(sizeof(sdt_wt_desc) == 4 * sizeof(void*) + 6 * sizeof(int32_t), wt_desc_size);
SDT_STATIC_ASSERT(offsetof(sdt_wt_desc, cout) == 4 * sizeof(void*), wt_desc_cout);
SDT_STATIC_ASSERT(offsetof(sdt_wt_desc, planes) == 4 * sizeof(void*) + 4 * sizeof(int32_t), wt_desc_planes);
/* ten int32_t (an even number: the pointers behind them need no padding), six pointers */
SDT_STATIC_ASSERT(sizeof(sdt_chain1d_layer) == 10 * sizeof(int32_t) + 6 * sizeof(void*), chain1d_layer_size);
SDT_STATIC_ASSERT(offsetof(sdt_chain1d_layer, in_mode) == 6 * sizeof(int32_t), chain1d_layer_in_mode);
SDT_STATIC_ASSERT(offsetof(sdt_chain1d_layer, w) == 10 * sizeof(int32_t), chain1d_layer_w);
SDT_STATIC_ASSERT(offsetof(sdt_chain1d_layer, dx) == 10 * sizeof(int32_t) + 5 * sizeof(void*), chain1d_layer_dx);
/* int64_t, three double, four int32_t */
SDT_STATIC_ASSERT(sizeof(sdt_render_instance) == sizeof(int64_t) + 3 * sizeof(double) + 4 * sizeof(int32_t), render_instance_size);
SDT_STATIC_ASSERT(offsetof(sdt_render_instance, shift_x) == sizeof(int64_t) + 3 * sizeof(double), render_instance_shift_x);

int main(void) {
    sdt_conv_geom g;
    int rc;
    memset(&g, 0, sizeof g);
    if (sdt_abi_version() != 5 || sdt_abi_version() != SDT_ABI_VERSION) return 10;
    if (sizeof(sdt_conv_geom) != (17 + 3 * SDT_MAX_TAPS) * sizeof(int32_t)) return 11;
    if (sizeof(sdt_wt_desc) != 4 * sizeof(void*) + 6 * sizeof(int32_t)) return 12;
    rc = sdt_conv_taps_f32(NULL, NULL, NULL, NULL, &g, NULL); /* zero geometry -> argument error, message set */
    if (rc != SDT_ERR_ARG || strlen(sdt_last_error()) == 0) return 13;
    printf("last error: %s\n", sdt_last_error());
    rc = sdt_adam_step_f32(NULL, NULL, NULL, NULL, 0, NULL, 0.9f, 0.999f, 1e-8f, 0.f, 1.f, NULL, NULL);
    if (rc != SDT_ERR_ARG) return 14;
    if (sdt_set_conv_math(42) != SDT_ERR_ARG || sdt_get_conv_math() != SDT_MATH_F32) return 15;
    if (sdt_set_conv_math(SDT_MATH_BF16) != SDT_OK || sdt_get_conv_math() != SDT_MATH_BF16) return 16;
    if (sdt_set_conv_math(SDT_MATH_F32) != SDT_OK) return 17;
    /* the bf16-storage entry points: a NULL geometry is unsupported (0 / -1), a NULL tensor an argument error */
    if (sdt_convsk_supported_t(NULL, 1, SDT_BF16) != 0 || sdt_convsk_plan_bytes_t(NULL, 1, SDT_BF16) != -1) return 18;
    if (sdt_convsk_dw_supported_t(NULL, SDT_BF16) != 0) return 19;
    rc = sdt_convsk_bf16(NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1u, NULL, NULL, 0, 0, 0, NULL);
    if (rc != SDT_ERR_ARG) return 20;
    rc = sdt_colnorm_fwd_t(NULL, SDT_BF16, NULL, SDT_BF16, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1, 1, 4, 1e-5f, 0.1f, 0.2f, 0, NULL);
    if (rc != SDT_ERR_ARG) return 21;
    if (sdt_convsk_set_spin_limit(sdt_convsk_get_spin_limit()) != SDT_OK) return 22;
    /* the Conv1d chain: the wiring is validated on the host before anything is launched */
    {
        sdt_chain1d_layer L[2];
        float dummy = 0.f;
        unsigned words[2] = {0u, 0u};
        memset(L, 0, sizeof L);
        if (sizeof(sdt_chain1d_layer) != 10 * sizeof(int32_t) + 6 * sizeof(void*)) return 23;
        L[0].Ti = 64, L[0].To = 64, L[0].Cin = 288, L[0].k = 3, L[0].stride = 1, L[0].pad = 1, L[0].in_mode = SDT_CHAIN_PLAIN, L[0].src_a = L[0].src_b = -1;
        L[1] = L[0];
        L[1].Cin = 256, L[1].in_mode = SDT_CHAIN_NORM, L[1].src_a = 1; /* a block cannot read itself */
        L[0].w = L[1].w = &dummy, L[0].y = L[1].y = &dummy;
        rc = sdt_chain1d_fwd_f32(L, 2, &dummy, &dummy, 4, 0.2f, 1e-5f, SDT_MATH_F32, words, words + 1, NULL);
        if (rc != SDT_ERR_ARG) return 24;
        L[1].src_a = 0, L[1].k = 5, L[1].pad = 2; /* no K loop was built for a 5-tap block */
        if (sdt_chain1d_supported(L, 2, 4) != 0) return 25;
        if (sdt_chain1d_bwd_f32(NULL, 2, &dummy, 4, 0.2f, 1e-5f, 1, SDT_MATH_F32, words, words + 1, NULL) != SDT_ERR_ARG) return 26;
    }
    puts("C ABI OK");
    return 0;
}
