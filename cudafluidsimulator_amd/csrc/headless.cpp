// Stand-in for the GLUT front end when ./sph is built without display.cpp.
// It defines the two globals the simulator links against (display.cpp:19-20)
// and a startVisualization() that steps the simulation without a window.
// Never linked together with display.cpp (duplicate symbols by design).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sha256.h"
#include "simulator.h"

bool mouseClicked = false;
int2 clickCoords;

extern "C" void glutInit(int *, char **) {}

// SPH_FREE_SHADE=speed|density|pressure: the field (SPH_FIELD_* of sph_c_api.h) that colours the frames;
// unset: -1, the reference's flat blue.  An unknown name is reported and gives the flat frame.
static int shade_field() {
    const char *e = getenv("SPH_FREE_SHADE");
    if (!e) return -1;
    const char *names[3] = {"speed", "density", "pressure"};
    for (int k = 0; k < 3; ++k)
        if (!strcmp(e, names[k])) return k;
    fprintf(stderr, "sph: SPH_FREE_SHADE=%s is not speed, density or pressure -- writing flat frames\n", e);
    return -1;
}

// SPH_FREE_FRAMES_DIR=<dir>: what the window would have shown after frame f, as <dir>/frame_%04d.ppm (binary P6)
static bool write_frame(Simulator *simulator, const char *dir, int f, int field) {
    int w = 0, h = 0;
    const unsigned char *rgb = field < 0 ? simulator->renderFrame(&w, &h) : simulator->renderField(field, &w, &h);
    if (!rgb) return false;
    char name[32];
    snprintf(name, sizeof name, "/frame_%04d.ppm", f);
    const std::string path = std::string(dir) + name;
    FILE *out = fopen(path.c_str(), "wb");
    if (!out) {
        fprintf(stderr, "sph: cannot write %s\n", path.c_str());
        return false;
    }
    fprintf(out, "P6\n%d %d\n255\n", w, h);
    const size_t bytes = (size_t)w * (size_t)h * 3;
    const bool ok = fwrite(rgb, 1, bytes, out) == bytes;
    return (fclose(out) == 0) && ok;
}

void startVisualization(Simulator *simulator) {
    int frames = 100;
    if (const char *e = getenv("SPH_FREE_FRAMES")) frames = atoi(e);
    const char *framesDir = getenv("SPH_FREE_FRAMES_DIR");
    if (framesDir && !*framesDir) framesDir = NULL;
    int every = 1;
    if (const char *e = getenv("SPH_FREE_FRAME_EVERY")) every = atoi(e) > 0 ? atoi(e) : 1;
    const int field = framesDir ? shade_field() : -1;
    fprintf(stderr, "sph: built without GLUT -- running %d frames headless\n", frames);
    for (int f = 0; f < frames; ++f) {
        if (f == frames / 2 && getenv("SPH_FREE_CLICK")) {
            mouseClicked = true;
            clickCoords = make_int2(400, 300);
        }
        simulator->simulate();
        if (framesDir && f % every == 0 && !write_frame(simulator, framesDir, f, field)) framesDir = NULL;
    }
    const float3 *p = simulator->getPosition();
    if (p && simulator->settings->numParticles > 0)
        printf("particle 0 after %d frames: (%f, %f, %f)\n", frames, p[0].x, p[0].y, p[0].z);
    if (p && getenv("SPH_PRINT_SHA256"))
        printf("positions_sha256 %s\n",
               sha256_hex(p, (size_t)simulator->settings->numParticles * sizeof(float3)).c_str());
}
