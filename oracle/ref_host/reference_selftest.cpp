/* Sanitizer self-test of the reference's simulator run on the host (test infrastructure;
 * tests/test_reference_pin_cpu.py).  Built by `make -C oracle ref-sanitize REF_SRC=...` from this file,
 * reference_driver.cpp and the reference's simulator.cu compiled as C++ against ref_host/cuda_runtime.h, all with
 * -fsanitize=address,undefined.  Two small states that stay inside the grid: the reference's own grid
 * initialiser, and a seeded cloud with velocities, a build schedule and a click.  Exits 0 if nothing was reported.
 * Leak checking is off where this runs: the reference's setup() never frees its staging array. */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "simulator.h"

extern "C" {
void *ref_create(const void *settings, int bytes);
void ref_setup(void *h);
int ref_upload(void *h, const float *pos, const float *vel);
int ref_set_schedule(void *h, const int32_t *order, int n);
int ref_step(void *h, int click, int mouse_x, int mouse_y);
void ref_download(void *h, float *pos, float *vel, float *rho, float *prs, float *force);
void ref_get_position(void *h, float *out);
void ref_destroy(void *h);
}

static unsigned lcg(unsigned *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

static Settings settings_for(int n) {
    /* h = 0.1, a box of 10 with 100^3 cells, dt = 0.01, as oracle_make_settings() forms them */
    const float h = .1f;
    const float v = 45.f / (PI * (float)std::pow((double)h, 6.0)), d = 315.f / (64.f * PI * (float)std::pow((double)h, 9.0));
    Settings s = {false, n, h, v, d, 10.f, 100, (float).01};
    return s;
}

static int run(int n, bool upload, unsigned seed) {
    Settings s = settings_for(n);
    void *h = ref_create(&s, (int)sizeof s);
    if (!h) return 1;
    ref_setup(h);
    std::vector<float> pos(3 * (size_t)n), vel(3 * (size_t)n), rho(n), prs(n), frc(3 * (size_t)n);
    if (upload) {
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) {
                pos[3 * i + a] = 4.0f + 1.5f * (float)(lcg(&seed) % 100000) / 100000.f;   /* ~30 rows per cell */
                vel[3 * i + a] = (float)((int)(lcg(&seed) % 2001) - 1000) / 500.f;
            }
        if (ref_upload(h, pos.data(), vel.data())) return 2;
    }
    std::vector<int32_t> order(n);
    for (int k = 0; k < 3; ++k) {
        if (k == 1) {                          /* a schedule: evens, then odds */
            int at = 0;
            for (int i = 0; i < n; i += 2) order[at++] = i;
            for (int i = 1; i < n; i += 2) order[at++] = i;
            if (ref_set_schedule(h, order.data(), n)) return 3;
        }
        if (ref_step(h, upload && k == 1, 400, 300)) return 4;
    }
    ref_download(h, pos.data(), vel.data(), rho.data(), prs.data(), frc.data());
    std::vector<float> host(3 * (size_t)n);
    ref_get_position(h, host.data());
    double sum = 0;
    for (int i = 0; i < n; ++i) sum += pos[3 * i] + rho[i] + host[3 * i + 1];
    std::printf("n=%d %s: ok (checksum %.6g)\n", n, upload ? "uploaded cloud, schedule, click" : "grid initialiser", sum);
    ref_destroy(h);
    return 0;
}

int main() {
    if (int rc = run(777, false, 1u)) return rc;
    if (int rc = run(3000, true, 2u)) return rc;
    std::puts("reference self-test: done");
    return 0;
}
