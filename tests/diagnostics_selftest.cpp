// Stand-alone driver of the diagnostics' two pure host functions (sph_diagnostics_add, sph_diagnostics_values),
// built by tests/test_diagnostics_cpu.py together with csrc/sph_diag_values.cpp under AddressSanitizer +
// UndefinedBehaviorSanitizer and run once.  Prints "name value" lines the test holds against Python's own numbers.
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "sph_c_api.h"

static SphDiagnosticsRaw one_row(int64_t lo_word, int64_t hi_word, uint32_t bits) {
    SphDiagnosticsRaw r;
    memset(&r, 0, sizeof r);
    r.struct_size = (int32_t)sizeof r;
    r.n = 1;
    for (int k = 0; k < SPH_DIAG_SUMS; ++k) {
        r.sum[k].lo = (uint64_t)lo_word;
        r.sum[k].hi = hi_word;
    }
    for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) r.min_bits[k] = r.max_bits[k] = bits;
    r.hist_field = -1;
    return r;
}

static void print_values(const char *tag, const SphDiagnosticsRaw &r) {
    SphSettings s;
    memset(&s, 0, sizeof s);
    s.h = 0.1f;
    s.timestep = 0.004f;
    SphDiagnostics d;
    const int rc = sph_diagnostics_values(&r, &s, &d);
    printf("%s_rc %d\n", tag, rc);
    printf("%s_sum_lo %" PRIu64 "\n%s_sum_hi %" PRId64 "\n", tag, r.sum[SPH_DIAG_SUM_V2].lo, tag, r.sum[SPH_DIAG_SUM_V2].hi);
    printf("%s_kinetic %a\n%s_potential %a\n%s_com_x %a\n%s_momentum_x %a\n%s_mass %a\n%s_cfl %a\n", tag, d.kinetic, tag,
           d.potential, tag, d.com[0], tag, d.momentum[0], tag, d.mass, tag, d.cfl);
}

int main() {
    printf("sizeof_options %zu\nsizeof_sum128 %zu\nsizeof_raw %zu\nsizeof_values %zu\n", sizeof(SphDiagnosticsOptions),
           sizeof(SphSum128), sizeof(SphDiagnosticsRaw), sizeof(SphDiagnostics));
    printf("raw_n %zu\nraw_sum %zu\nraw_min_bits %zu\nraw_max_bits %zu\nraw_saturated %zu\nraw_hist_field %zu\n"
           "raw_hist_lo_bits %zu\nraw_hist_hi_bits %zu\nraw_hist %zu\n",
           offsetof(SphDiagnosticsRaw, n), offsetof(SphDiagnosticsRaw, sum), offsetof(SphDiagnosticsRaw, min_bits),
           offsetof(SphDiagnosticsRaw, max_bits), offsetof(SphDiagnosticsRaw, saturated), offsetof(SphDiagnosticsRaw, hist_field),
           offsetof(SphDiagnosticsRaw, hist_lo_bits), offsetof(SphDiagnosticsRaw, hist_hi_bits), offsetof(SphDiagnosticsRaw, hist));
    printf("values_n %zu\nvalues_mass %zu\nvalues_com %zu\nvalues_momentum %zu\nvalues_kinetic %zu\nvalues_potential %zu\n"
           "values_mean_rho %zu\nvalues_mean_prs %zu\nvalues_min_rho %zu\nvalues_max_rho %zu\nvalues_max_speed %zu\n"
           "values_cfl %zu\nvalues_box_min %zu\nvalues_box_max %zu\nvalues_saturated %zu\n",
           offsetof(SphDiagnostics, n), offsetof(SphDiagnostics, mass), offsetof(SphDiagnostics, com),
           offsetof(SphDiagnostics, momentum), offsetof(SphDiagnostics, kinetic), offsetof(SphDiagnostics, potential),
           offsetof(SphDiagnostics, mean_rho), offsetof(SphDiagnostics, mean_prs), offsetof(SphDiagnostics, min_rho),
           offsetof(SphDiagnostics, max_rho), offsetof(SphDiagnostics, max_speed), offsetof(SphDiagnostics, cfl),
           offsetof(SphDiagnostics, box_min), offsetof(SphDiagnostics, box_max), offsetof(SphDiagnostics, saturated));

    // a 128-bit carry: 2^20 terms of INT64_MAX, by doubling
    SphDiagnosticsRaw big = one_row(INT64_MAX, 0, 0x40400000u /* 3.0f */);
    for (int k = 0; k < 20; ++k) {
        const SphDiagnosticsRaw copy = big;
        printf("carry_add_rc %d\n", sph_diagnostics_add(&big, &copy));
    }
    printf("carry_n %" PRId64 "\n", big.n);
    print_values("carry", big);

    // negative sums: 3 terms of -1 (q(-2^-33)), and 2^20 terms of INT64_MIN
    SphDiagnosticsRaw neg = one_row(-1, -1, 0xBF800000u /* -1.0f */);
    const SphDiagnosticsRaw neg1 = neg;
    sph_diagnostics_add(&neg, &neg1);
    sph_diagnostics_add(&neg, &neg1);
    print_values("neg", neg);
    SphDiagnosticsRaw low = one_row(INT64_MIN, -1, 0x3F800000u);
    for (int k = 0; k < 20; ++k) {
        const SphDiagnosticsRaw copy = low;
        sph_diagnostics_add(&low, &copy);
    }
    print_values("low", low);

    // ties of the 128-bit -> double conversion: 2^53 + 1 (to even: down), 2^53 + 3 (up), then a part without rows
    SphDiagnosticsRaw tie = one_row((int64_t)((1ll << 53) + 1), 0, 0x3F800000u);
    print_values("tie_down", tie);
    tie = one_row((int64_t)((1ll << 53) + 3), 0, 0x3F800000u);
    print_values("tie_up", tie);
    SphDiagnosticsRaw empty = one_row(0, 0, 0);
    empty.n = 0;
    for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) empty.min_bits[k] = 0x7F800000u, empty.max_bits[k] = 0xFF800000u;
    print_values("empty", empty);
    printf("empty_add_rc %d\n", sph_diagnostics_add(&empty, &tie));
    printf("empty_then_bytes_equal %d\n", memcmp(&empty, &tie, sizeof tie) == 0);

    // what must be refused
    SphDiagnosticsRaw other = tie;
    other.hist_field = SPH_FIELD_SPEED;
    printf("field_mismatch_rc %d\n", sph_diagnostics_add(&other, &tie));
    other = tie;
    other.hist_lo_bits = 1;
    printf("range_mismatch_rc %d\n", sph_diagnostics_add(&other, &tie));
    printf("null_rc %d\n", sph_diagnostics_add(nullptr, &tie));
    return 0;
}
