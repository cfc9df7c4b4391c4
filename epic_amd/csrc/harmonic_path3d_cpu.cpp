// harmonic_path3d_cpu.cpp -- consumers and sparse edits of a 3-D field on the host (include/epic_hip.h, "3-D fields").
//
// The reference has no 3-D walker: its streamline code (libepic/src/harmonic/harmonic_path_cpu.cpp:41-232, restated in
// harmonic_path_cpu.cpp of this directory) is 2-D only.  This file is that rule with a third axis, generalised operation by
// operation: the usable test, the interpolation, the normalised central-difference gradient, the "stuck" detector and the
// gradient-ascent loop keep the 2-D code's types, order of operations and quirks (alpha in [0.5, 1.5), std::pow on a float
// evaluated in double, the unsigned product in the length bound).  The third axis is always the LAST operand:
//   trilinear = (1 - gamma) * front + gamma * back,  front / back = the 2-D bilinear on planes z0 / z1;
//   norm      = (float)sqrt(pow(gx, 2) + pow(gy, 2) + pow(gz, 2)), summed left to right in double;
//   distance  = the same three-term form.
// With that association a field that is constant along z, walked from an integer z with cdPrecision = 0.5, reproduces the 2-D
// walk bit for bit (gamma is exactly 1 or 0.5, gz is exactly +0, adding +0.0 to the double sums changes nothing): the anchor to
// the reference, tests/test_path3d_cpu.py.  The device walk (field_3d.hip) restates this file the same way.
//
// Axes: cell (x0, x1, x2) of m = {m0, m1, m2} sits at u[(x0 * m1 + x1) * m2 + x2] (harmonic_cpu.cpp:102).  A point is (x, y, z)
// in cell units: x along m[2] (columns), y along m[1] (rows), z along m[0] (planes) -- the 2-D convention with z as the slowest
// axis.  Two deliberate differences from the 2-D code, both where it reads outside its arrays: its loop reads locked[] at the cell
// of the newest point without a bounds test (a step longer than a cell can leave the grid) -- here a point outside the grid ends the
// walk; and its interpolation wraps an index at a sample exactly half a cell outside a usable face cell -- here reads are clamped
// to the nearest cell.  Both are what the device does (tests/test_path3d_sanitize.py runs these cases under AddressSanitizer).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../include/epic/epic_abi.h"
#include "../../include/epic_hip.h"

namespace {

using epic::Harmonic;

constexpr unsigned kStuckHistory = 5;  // PATH_STUCK_HISTORY_LENGTH, harmonic_path_cpu.cpp:39

struct Field3 {
    unsigned nx, ny, nz;  // columns (m[2]), rows (m[1]), planes (m[0])
    const unsigned *locked;
    const float *u;
    size_t cell(unsigned x, unsigned y, unsigned z) const { return ((size_t)z * ny + y) * nx + x; }
    // clamped, as on the device: the one point where the 2-D code reads outside its arrays -- a sample exactly half a cell outside a
    // goal cell of a face, where to_index(x - 0.5f) wraps -- reads the nearest cell instead
    float at(unsigned x, unsigned y, unsigned z) const { return u[cell(std::min(x, nx - 1u), std::min(y, ny - 1u), std::min(z, nz - 1u))]; }
    unsigned lock(unsigned x, unsigned y, unsigned z) const { return locked[cell(x, y, z)]; }
    bool inside(unsigned x, unsigned y, unsigned z) const { return x < nx && y < ny && z < nz; }
};

// float -> unsigned as x86-64 compiles the 2-D code's (unsigned)(float): a 64-bit signed truncation whose low word is kept, so a value
// below -1 wraps to a huge index (and fails the bounds test) -- spelled out, so that it is the same on every host and on the device
inline unsigned to_index(float v) { return (unsigned)(long long)v; }

// outside the grid, or a locked cell with u < 0 (an obstacle; goals are locked with u == 0)
bool usable(const Field3 &f, float x, float y, float z)
{
    const unsigned cx = to_index(x + 0.5f), cy = to_index(y + 0.5f), cz = to_index(z + 0.5f);
    if (!f.inside(cx, cy, cz)) return false;
    if (f.lock(cx, cy, cz) != 1) return true;
    return !(f.at(cx, cy, cz) < 0.0f);
}

// Interpolation between the eight cell centres around (x, y, z); only called on usable points.
float trilinear(const Field3 &f, float x, float y, float z)
{
    const unsigned x0 = to_index(x - 0.5f), x1 = to_index(x + 0.5f);
    const unsigned y0 = to_index(y - 0.5f), y1 = to_index(y + 0.5f);
    const unsigned z0 = to_index(z - 0.5f), z1 = to_index(z + 0.5f);
    const float alpha = x - x0, beta = y - y0, gamma = z - z0;
    const float top0 = (1.0f - alpha) * f.at(x0, y0, z0) + alpha * f.at(x1, y0, z0);
    const float bottom0 = (1.0f - alpha) * f.at(x0, y1, z0) + alpha * f.at(x1, y1, z0);
    const float front = (1.0f - beta) * top0 + beta * bottom0;
    const float top1 = (1.0f - alpha) * f.at(x0, y0, z1) + alpha * f.at(x1, y0, z1);
    const float bottom1 = (1.0f - alpha) * f.at(x0, y1, z1) + alpha * f.at(x1, y1, z1);
    const float back = (1.0f - beta) * top1 + beta * bottom1;
    return (1.0f - gamma) * front + gamma * back;
}

const char *const kPathName = "epic_hip_compute_path_3d_cpu";
const char *const kGradientName = "epic_hip_compute_gradient_3d_cpu";
const char *const kPotentialName = "epic_hip_compute_potential_3d_cpu";

int potential(const Field3 &f, float x, float y, float z, float &out)
{
    if (!usable(f, x, y, z)) {
        fprintf(stderr, "Error[%s]: %s\n", kPotentialName, "Invalid location.");
        return EPIC_ERROR_INVALID_LOCATION;
    }
    out = trilinear(f, x, y, z);
    return EPIC_SUCCESS;
}

// Central differences at +-cd (samples in the order x-, x+, y-, y+, z-, z+), normalised to unit length; the norm in double.
int gradient(const Field3 &f, float x, float y, float z, float cd, float &gx, float &gy, float &gz)
{
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int rc = potential(f, x - cd, y, z, v[0]);
    rc += potential(f, x + cd, y, z, v[1]);
    rc += potential(f, x, y - cd, z, v[2]);
    rc += potential(f, x, y + cd, z, v[3]);
    rc += potential(f, x, y, z - cd, v[4]);
    rc += potential(f, x, y, z + cd, v[5]);
    if (rc != EPIC_SUCCESS) {
        fprintf(stderr, "Error[%s]: %s\n", kGradientName, "Failed to compute potential values.");
        return EPIC_ERROR_INVALID_GRADIENT;
    }
    gx = (v[1] - v[0]) / (2.0f * cd);
    gy = (v[3] - v[2]) / (2.0f * cd);
    gz = (v[5] - v[4]) / (2.0f * cd);
    const float norm = (float)std::sqrt(std::pow(gx, 2) + std::pow(gy, 2) + std::pow(gz, 2));  // the 2-D overloads: double
    gx /= norm;
    gy /= norm;
    gz /= norm;
    return EPIC_SUCCESS;
}

// True when the newest point came back to within stepSize / 2 of one of the previous kStuckHistory points.
bool stuck(const std::vector<float> &p, float stepSize)
{
    const unsigned n = (unsigned)p.size();
    if (n % 3 != 0) return true;
    if (n == 0) return false;
    const float x = p[n - 3], y = p[n - 2], z = p[n - 1];
    const int floor_i = std::max(0, (int)n - 3 * (int)kStuckHistory - 3);
    for (unsigned i = n - 3; i > (unsigned)floor_i; i -= 3) {
        const float dx = x - p[i - 3], dy = y - p[i - 2], dz = z - p[i - 1];
        const float dist = (float)std::sqrt(std::pow(dx, 2) + std::pow(dy, 2) + std::pow(dz, 2));
        if (dist < stepSize / 2.0f) return true;
    }
    return false;
}

// Follow the gradient from (x, y, z) until a locked cell is entered, the grid is left, the walk gets stuck, or the length bound
// is hit: the loop of harmonic_path_cpu.cpp:154-221.
int follow(const Field3 &f, float x, float y, float z, float stepSize, float cd, unsigned max_points, unsigned &k, float *&path)
{
    if (!usable(f, x, y, z)) {
        fprintf(stderr, "Error[%s]: %s\n", kPathName, "Invalid location.");
        return EPIC_ERROR_INVALID_LOCATION;
    }
    std::vector<float> pts;
    pts.push_back(x);
    pts.push_back(y);
    pts.push_back(z);
    unsigned cx = to_index(x + 0.5f), cy = to_index(y + 0.5f), cz = to_index(z + 0.5f);
    while (f.inside(cx, cy, cz) && f.lock(cx, cy, cz) != 1 && !stuck(pts, stepSize) && pts.size() / 3 < max_points) {
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        if (gradient(f, x, y, z, cd, gx, gy, gz) != EPIC_SUCCESS) {
            fprintf(stderr, "Error[%s]: %s\n", kPathName, "Could not compute gradient.");
            return EPIC_ERROR_INVALID_GRADIENT;
        }
        x += gx * stepSize;
        y += gy * stepSize;
        z += gz * stepSize;
        pts.push_back(x);
        pts.push_back(y);
        pts.push_back(z);
        cx = to_index(x + 0.5f);
        cy = to_index(y + 0.5f);
        cz = to_index(z + 0.5f);
    }
    // two points or fewer: the gradient was degenerate, i.e. the field is not relaxed enough here
    if (pts.size() / 3 <= 2) {
        fprintf(stderr, "Error[%s]: %s\n", kPathName, "Could not compute a valid path.");
        return EPIC_ERROR_INVALID_PATH;
    }
    k = (unsigned)(pts.size() / 3);
    path = new float[3 * (size_t)k];  // released with harmonic_free_path_cpu (delete[])
    for (size_t i = 0; i < 3 * (size_t)k; i++) path[i] = pts[i];
    return EPIC_SUCCESS;
}

bool valid(const Harmonic *h) { return h && h->m && h->u && h->locked && h->n == 3; }

Field3 field_of(const Harmonic *h) { return Field3{h->m[2], h->m[1], h->m[0], h->locked, h->u}; }

}  // namespace

extern "C" {

int epic_hip_compute_potential_3d_cpu(Harmonic *harmonic, float x, float y, float z, float *potential_out)
{
    if (!valid(harmonic) || potential_out == nullptr) {
        fprintf(stderr, "Error[%s]: %s\n", kPotentialName, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    return potential(field_of(harmonic), x, y, z, *potential_out);
}

int epic_hip_compute_gradient_3d_cpu(Harmonic *harmonic, float x, float y, float z, float cdPrecision, float *gx, float *gy,
                                     float *gz)
{
    if (!valid(harmonic) || gx == nullptr || gy == nullptr || gz == nullptr) {
        fprintf(stderr, "Error[%s]: %s\n", kGradientName, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    return gradient(field_of(harmonic), x, y, z, cdPrecision, *gx, *gy, *gz);
}

int epic_hip_compute_path_3d_cpu(Harmonic *harmonic, float x, float y, float z, float stepSize, float cdPrecision,
                                 unsigned int maxLength, unsigned int *k, float **path)
{
    if (!valid(harmonic) || k == nullptr || path == nullptr || *path != nullptr) {
        fprintf(stderr, "Error[%s]: %s\n", kPathName, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    // the 2-D loop compares size() with the unsigned product 2 * maxLength (harmonic_path_cpu.cpp:185): in points, that is
    return follow(field_of(harmonic), x, y, z, stepSize, cdPrecision, (2u * maxLength) / 2u, *k, *path);
}

// harmonic_utilities_set_cells_2d_cpu (reference harmonic_utilities_cpu.cpp:38-76) on (x, y, z) triples.
int epic_hip_set_cells_3d_cpu(Harmonic *harmonic, unsigned int k, const unsigned int *v, const unsigned int *types)
{
    static const char *fn = "epic_hip_set_cells_3d_cpu";
    if (!valid(harmonic) || k == 0 || v == nullptr || types == nullptr) {
        fprintf(stderr, "Error[%s]: %s\n", fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    const unsigned nz = harmonic->m[0], ny = harmonic->m[1], nx = harmonic->m[2];
    for (unsigned i = 0; i < k; i++) {
        const unsigned x = v[3 * (size_t)i], y = v[3 * (size_t)i + 1], z = v[3 * (size_t)i + 2];
        if (z >= nz || y >= ny || x >= nx) {
            fprintf(stderr, "Warning[%s]: %s\n", fn, "Provided vector has invalid values outside area.");
            continue;
        }
        const size_t cell = ((size_t)z * ny + y) * nx + x;
        switch (types[i]) {
        case EPIC_CELL_TYPE_GOAL:
            harmonic->u[cell] = EPIC_LOG_SPACE_GOAL;
            harmonic->locked[cell] = 1;
            break;
        case EPIC_CELL_TYPE_OBSTACLE:
            harmonic->u[cell] = EPIC_LOG_SPACE_OBSTACLE;
            harmonic->locked[cell] = 1;
            break;
        case EPIC_CELL_TYPE_FREE:
            harmonic->u[cell] = EPIC_LOG_SPACE_FREE;
            harmonic->locked[cell] = 0;
            break;
        default:
            fprintf(stderr, "Warning[%s]: %s\n", fn, "Type is invalid. No change made.");
            break;
        }
    }
    return EPIC_SUCCESS;
}

}  // extern "C"
