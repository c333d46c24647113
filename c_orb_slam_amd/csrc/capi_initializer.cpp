// capi_initializer.cpp -- extern "C" Initializer_* (include/orbslam_gpu.h), reference
// include/Initializer.h and src/Initializer.cc.
// Host pointers only.  Normalize runs here (its float sums are sequential in the reference);
// a call packs the parameters, the matched pixel and normalised coordinates into one staging
// block (one H2D copy), runs the four kernels of initializer.hip on the handle's stream and
// fetches one result block (one D2H copy).
#include <cmath>
#include <cstring>
#include <vector>

#include "initializer.hpp"
#include "orb_common.hpp"
#include "pnp.hpp"

using orbgpu::InitDev;
using orbgpu::InitOut;
using orbgpu::InitParams;
using orbgpu::InitState;

struct Initializer_t {
    hipStream_t stream = nullptr;
    int n1 = 0, iterations = 0;
    float sigma = 0, K[9], T1[9];
    std::vector<float> keys1, pn1;   // n1 x 2: pixels, normalised
    uint8_t* dev = nullptr;          // staging | work | result, grown on demand
    size_t cap = 0;
    bool timing = false, timed = false;
    hipEvent_t ev[5] = {};
    float ms[4] = {};
};

namespace {

size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

bool all_finite(const float* v, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// Initializer::Normalize (Initializer.cc:752-805) over every key of a frame: sequential float
// sums, sX = 1.0 / meanDevX rounded to float, T = [sX 0 -meanX*sX; 0 sY -meanY*sY; 0 0 1]
void normalize(const float* keys, int n, std::vector<float>& pts, float* T) {
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) {
        meanX += keys[2 * i];
        meanY += keys[2 * i + 1];
    }
    meanX = meanX / (float)n;
    meanY = meanY / (float)n;
    float meanDevX = 0, meanDevY = 0;
    pts.resize((size_t)n * 2);
    for (int i = 0; i < n; i++) {
        pts[2 * i] = keys[2 * i] - meanX;
        pts[2 * i + 1] = keys[2 * i + 1] - meanY;
        meanDevX += std::fabs(pts[2 * i]);
        meanDevY += std::fabs(pts[2 * i + 1]);
    }
    meanDevX = meanDevX / (float)n;
    meanDevY = meanDevY / (float)n;
    const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
    for (int i = 0; i < n; i++) {
        pts[2 * i] = pts[2 * i] * sX;
        pts[2 * i + 1] = pts[2 * i + 1] * sY;
    }
    const float t[9] = {sX, 0, -meanX * sX, 0, sY, -meanY * sY, 0, 0, 1};
    std::memcpy(T, t, sizeof(t));
}

}  // namespace

extern "C" {

int Initializer_create(const float* K, int n1, const float* keys1, float sigma, int iterations, Initializer_h* out) {
    if (!out || !K || n1 < 0 || (n1 > 0 && !keys1) || iterations < 1 || !(sigma > 0) || !std::isfinite(sigma))
        return ORB_E_INVALID;
    if (!all_finite(K, 9) || !all_finite(keys1, (size_t)n1 * 2)) return ORB_E_INVALID;
    *out = nullptr;
    if (no_device()) return ORB_E_NODEVICE;
    Initializer_t* h = new Initializer_t();
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return ORB_E_HIP;
    }
    for (int i = 0; i < 5; i++)
        if (hipEventCreate(&h->ev[i]) != hipSuccess) {
            Initializer_destroy(h);
            return ORB_E_HIP;
        }
    h->n1 = n1;
    h->iterations = iterations;
    h->sigma = sigma;
    std::memcpy(h->K, K, sizeof(h->K));
    h->keys1.assign(keys1, keys1 + (size_t)n1 * 2);
    normalize(h->keys1.data(), n1, h->pn1, h->T1);
    *out = h;
    return ORB_OK;
}

int Initializer_destroy(Initializer_h h) {
    if (!h) return ORB_E_INVALID;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (int i = 0; i < 5; i++)
        if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    if (h->dev) (void)hipFree(h->dev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return ORB_OK;
}

int Initializer_Initialize(Initializer_h h, int n2, const float* keys2, const int32_t* matches12, orb_rng* rng,
                           float* R21, float* t21, float* vP3D, uint8_t* vbTriangulated, int* ok,
                           orb_init_info* info) {
    if (n2 < 0 || !keys2 || !matches12 || !rng || !R21 || !t21 || !vP3D || !vbTriangulated || !ok)
        return ORB_E_INVALID;
    if (rng->f < 0 || rng->f >= 31 || rng->r < 0 || rng->r >= 31) return ORB_E_INVALID;   // not a seeded stream
    if (!all_finite(keys2, (size_t)n2 * 2)) return ORB_E_INVALID;
    // the handle is looked at last: without one the call is malformed where a device exists and
    // has no device to run on otherwise; the matches are checked against its n1
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    const int n1 = h->n1, iterations = h->iterations;
    int N = 0;
    for (int i = 0; i < n1; i++) {
        if (matches12[i] >= n2) return ORB_E_INVALID;
        N += matches12[i] >= 0;
    }
    if (N < 8) return ORB_E_INVALID;
    if (n1 >= (1 << 22)) return ORB_E_CAPACITY;   // RandomInt's integer form (ransac_dev.hpp) and the int indices

    // staging block: parameters, pixel and normalised coordinates, frame-1 key of each match
    std::vector<float> pn2;
    InitParams P;
    std::memset(&P, 0, sizeof(P));
    float T2[9];
    normalize(keys2, n2, pn2, T2);
    P.rng = *rng;
    std::memcpy(P.K, h->K, sizeof(P.K));
    std::memcpy(P.T1, h->T1, sizeof(P.T1));
    orbgpu::inv3(T2, P.T2inv);
    orbgpu::tr3(T2, P.T2t);
    P.sigma = h->sigma;
    P.iterations = iterations;
    P.N = N;
    P.n1 = n1;
    const size_t oPar = 0, oPx = oPar + al(sizeof(P)), oPn = oPx + al((size_t)N * 16), oFirst = oPn + al((size_t)N * 16),
                 inEnd = oFirst + al((size_t)N * 4);
    std::vector<uint8_t> in(inEnd);
    std::memcpy(in.data() + oPar, &P, sizeof(P));
    float* px = (float*)(in.data() + oPx);
    float* pn = (float*)(in.data() + oPn);
    int* first = (int*)(in.data() + oFirst);
    for (int i = 0, k = 0; i < n1; i++) {
        const int j = matches12[i];
        if (j < 0) continue;
        px[4 * k] = h->keys1[2 * i];
        px[4 * k + 1] = h->keys1[2 * i + 1];
        px[4 * k + 2] = keys2[2 * j];
        px[4 * k + 3] = keys2[2 * j + 1];
        pn[4 * k] = h->pn1[2 * i];
        pn[4 * k + 1] = h->pn1[2 * i + 1];
        pn[4 * k + 2] = pn2[2 * j];
        pn[4 * k + 3] = pn2[2 * j + 1];
        first[k++] = i;
    }
    // work: scores, matrices, state, keys, per-hypothesis points and flags
    const size_t wScores = inEnd, wMats = wScores + al((size_t)iterations * 8),
                 wState = wMats + al((size_t)iterations * 2 * 18 * 4), wKeys = wState + al(sizeof(InitState)),
                 wP3D = wKeys + al((size_t)N * 8 * 4), wGood = wP3D + al((size_t)n1 * 8 * 12),
                 workEnd = wGood + al((size_t)n1 * 8);
    // result block: info head, vP3D, vbTriangulated, the two masks
    const size_t rOut = 0, rP3D = rOut + al(sizeof(InitOut)), rTri = rP3D + al((size_t)n1 * 12),
                 rMH = rTri + al((size_t)n1), rMF = rMH + al((size_t)N), outEnd = rMF + al((size_t)N);
    const size_t need = workEnd + outEnd;
    if (need > h->cap) {
        if (h->dev) (void)hipFree(h->dev);
        h->dev = nullptr;
        h->cap = 0;
        if (hipMalloc((void**)&h->dev, need + need / 2) != hipSuccess) return ORB_E_HIP;
        h->cap = need + need / 2;
    }
    uint8_t* d = h->dev;
    uint8_t* dres = d + workEnd;
    hipStream_t s = h->stream;
    if (hipMemcpyAsync(d, in.data(), inEnd, hipMemcpyHostToDevice, s) != hipSuccess) return ORB_E_HIP;
    InitDev D;
    D.par = (const InitParams*)(d + oPar);
    D.px = (const float4*)(d + oPx);
    D.pn = (const float4*)(d + oPn);
    D.first = (const int*)(d + oFirst);
    D.scores = (float*)(d + wScores);
    D.mats = (float*)(d + wMats);
    D.st = (InitState*)(d + wState);
    D.keys = (uint32_t*)(d + wKeys);
    D.P3D = (float*)(d + wP3D);
    D.good = d + wGood;
    D.out = (InitOut*)(dres + rOut);
    D.vP3D = (float*)(dres + rP3D);
    D.tri = dres + rTri;
    D.maskH = dres + rMH;
    D.maskF = dres + rMF;
    if (orbgpu::initializer_launch(D, iterations, s, h->timing ? h->ev : nullptr)) return ORB_E_HIP;
    std::vector<uint8_t> res(outEnd);
    if (hipMemcpyAsync(res.data(), dres, outEnd, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
    if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
    if (h->timing) {
        for (int i = 0; i < 4; i++)
            if (hipEventElapsedTime(&h->ms[i], h->ev[i], h->ev[i + 1]) != hipSuccess) return ORB_E_HIP;
        h->timed = true;
    }
    // the stream position after the call: 8 draws per iteration
    for (int i = 0; i < 8 * iterations; i++) (void)orbgpu::rng_rand(rng);

    InitOut O;
    std::memcpy(&O, res.data() + rOut, sizeof(O));
    *ok = O.ok;
    if (O.ok) {
        std::memcpy(R21, O.R21, sizeof(O.R21));
        std::memcpy(t21, O.t21, sizeof(O.t21));
        std::memcpy(vP3D, res.data() + rP3D, (size_t)n1 * 12);
        std::memcpy(vbTriangulated, res.data() + rTri, (size_t)n1);
    }
    if (info) {
        info->SH = O.SH;
        info->SF = O.SF;
        info->use_H = O.use_H;
        info->best_it_H = O.best_it_H;
        info->best_it_F = O.best_it_F;
        std::memcpy(info->H21, O.H21, sizeof(O.H21));
        std::memcpy(info->F21, O.F21, sizeof(O.F21));
        info->n_hyp = O.n_hyp;
        std::memcpy(info->nGood, O.nGood, sizeof(O.nGood));
        std::memcpy(info->parallax, O.parallax, sizeof(O.parallax));
        info->chosen = O.chosen;
        if (info->inliersH) std::memcpy(info->inliersH, res.data() + rMH, (size_t)N);
        if (info->inliersF) std::memcpy(info->inliersF, res.data() + rMF, (size_t)N);
    }
    return ORB_OK;
}

int Initializer_enable_timing(Initializer_h h, int on) {
    if (!h) return ORB_E_INVALID;
    h->timing = on != 0;
    return ORB_OK;
}

int Initializer_last_timings(Initializer_h h, float* ms4) {
    if (!h || !ms4 || !h->timed) return ORB_E_INVALID;
    std::memcpy(ms4, h->ms, sizeof(h->ms));
    return ORB_OK;
}

}  // extern "C"
