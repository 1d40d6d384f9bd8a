// The walkers' random numbers: RANMAR, Gaussian1 and randexp1 of RandUtils.f90,
// on a strided per-walker view of the state (LDS or HBM).  Included by
// sampler.hip first of the Metropolis headers.
// (included inside namespace cmamd)
#pragma once

// strided per-walker column view (LDS: stride MB; HBM: stride W)
template <class T> struct Col {
    T *p;
    int s;
    __device__ T &operator[](int i) const { return p[(size_t)i * s]; }
};

// ------------------------------------------------------------ RNG (RandUtils.f90)

struct Rng {
    Col<double> u;  // u(1:97)
    double c;
    int i97, j97, iset;
    double gset;
    int nd = 0;     // draws so far (the lean chain writes back the ring entries they overwrote)
};

__device__ __forceinline__ double ranmar(Rng &r)
{   // RandUtils.f90:350-374
    double uni = r.u[r.i97 - 1] - r.u[r.j97 - 1];
    if (uni < 0.0) uni += 1.0;
    r.u[r.i97 - 1] = uni;
    if (--r.i97 == 0) r.i97 = 97;
    if (--r.j97 == 0) r.j97 = 97;
    r.nd++;
    const double cd = 7654321.0 / 16777216.0, cm = 16777213.0 / 16777216.0;
    r.c -= cd;
    if (r.c < 0.0) r.c += cm;
    uni -= r.c;
    if (uni < 0.0) uni += 1.0;
    return uni;
}

__device__ __forceinline__ double gaussian1(Rng &r)
{   // RandUtils.f90:156-178
    if (r.iset == 0) {
        double v1, v2, rr;
        do {
            v1 = 2.0 * ranmar(r) - 1.0;
            v2 = 2.0 * ranmar(r) - 1.0;
            rr = v1 * v1 + v2 * v2;
        } while (rr >= 1.0);
        const double fac = sqrt(-2.0 * log(rr) / rr);
        r.gset = v1 * fac;
        r.iset = 1;
        return v2 * fac;
    }
    r.iset = 0;
    return r.gset;
}

__device__ __forceinline__ float randexp1(Rng &r)
{   // RandUtils.f90:189-233, REAL(4) arithmetic (built with -ffp-contract=off)
    const float alog2 = 0.6931471805599453f, a = 5.7133631526454228f, b = 3.4142135623730950f;
    const float c = -1.6734053240284925f, p = 0.9802581434685472f, aa = 5.6005707569738080f;
    const float bb = 3.3468106480569850f, hh = 0.0026106723602095f, dd = 0.0857864376269050f;
    float u = (float)ranmar(r);
    while (u <= 0.0f) u = (float)ranmar(r);
    float g = c;
    u = u + u;
    while (u < 1.0f) {
        g = g + alog2;
        u = u + u;
    }
    u = u - 1.0f;
    if (u <= p) return g + aa / (bb - u);
    for (;;) {
        u = (float)ranmar(r);
        const float y = a / (b - u);
        const float up = (float)ranmar(r);
        const float bu = b - u;
        if ((up * hh + dd) * (bu * bu) <= expf(-(y + c))) return g + y;
    }
}
