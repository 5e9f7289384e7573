// geoac_lattice_list.h - the walk that geoac_stations.hip (ground stations) and geoac_lstations.hip (level stations) share: per (member, station)
// a list of the lattice triangles that hold the station, searched over n_planes planes of double4 corners (c0, c1, caller's own, present) with
// n_rays corners each.  A plane is a leg of the landing table on the ground (n_planes = n_legs) and a branch of the branch table for levels
// (n_planes = B).  The caller derives its kernel argument from ListDev and gives it three members, and nothing else:
//   const double4* plane(const Seg&)            the plane of a segment
//   bool admit(c0, c1, c2)                      a filter of its own on three present corners (false refuses the triangle)
//   void write_row(const Seg&, tri, const Tri&, r0, r1, r2, c0, c1, c2, row)      the row of a hit, row < M * n_sta * cap
// Its two kernels are one-line calls of list_count and list_rows; its table, its prep kernel, its state and its entry points stay its own.
//
// Two passes, one wave per list segment (member, station, plane, chunk of LIST_CHUNK lattice cells):
//   list_count   the hits of the segment.
//   list_rows    the same segments again.  A wave sums the integer counts of the segments before its own in the (member, station) list - its
//                base - and, when it has hits and the base is below cap, walks its chunk once more: per trip of 64 cells a ballot per
//                triangle of the cell and a prefix count give every hit its place.  Segments and triangles are walked in key order, so the
//                rows come out sorted by plane * n_tri + tri with no sort, no atomic and no floating-point reduction across threads: a list
//                is the same bits on every run.  Most segments have no hit and end after reading one count.
// One lane tests both triangles of a lattice cell (they share two of the cell's four corners).  There is no bounding-box reject in front of
// the cross products: in floating point it is not equivalent to the sign rule (a product difference can round to zero), and the three 32-byte
// corner loads it would need are the cost of the test anyway.  The ballots sit outside every lane-dependent branch: all 64 lanes of a wave
// reach them on every trip, the partial last trip included (a lane past the chunk's end votes no hit).
//
// The arithmetic is that of geoac_tri_rule.h, restated in tests/station_reference.py: contraction is off from here on.
//
// Index bounds, stated again at each load and store:
//   seg < M * n_sta * n_planes * n_chunks, so s < n_sta, p < n_planes, chunk < n_chunks, m < M, list < M * n_sta;  p * n_chunks + chunk < nseg;
//   cell < n_cells, so the corner rays a, b, c, d < n_theta * n_phi = n_rays (cell_rays; checked on the host: n_theta * n_phi == n_rays);
//   list row pos < cap (tested at the store).
#ifndef GEOAC_LATTICE_LIST_H_
#define GEOAC_LATTICE_LIST_H_

#include <hip/hip_runtime.h>
#include <vector>

#include "geoac_launch_int.h"
#include "geoac_tri_rule.h"

#pragma clang fp contract(off)

namespace {

const int LIST_CHUNK = 2048;                     // lattice cells per list segment: 32 trips of a wave

struct ListDev {
    const double* theta_ax; const double* phi_ax; // [n_theta], [n_phi] lattice axes [deg]
    const double* sta;                            // [n_sta][2]
    unsigned* cnt;                                // [M][n_sta][nseg]: hits per list segment
    unsigned* hits; double* rows;                 // the lists
    double edge2;                                 // edge_max * edge_max
    int spherical, periodic;
    int M, n_rays, n_theta, n_phi, n_sta, cap;
    int n_planes;                                 // planes per list
    int n_cells, n_chunks, nseg;                  // cells of the lattice, chunks per plane, segments per list = n_planes * n_chunks
};

// ray indices of the corners a, b, c, d of a cell, cell < n_cells: every one < n_theta * n_phi
__device__ inline void cell_rays(const ListDev& D, int cell, int* a, int* b, int* c, int* d){
    const int nt1 = D.n_theta - 1;
    const int i = cell % nt1, j = cell / nt1;            // i <= n_theta - 2; j <= n_phi - 1 under phi_periodic, else <= n_phi - 2
    const int jn = (j + 1 == D.n_phi) ? 0 : j + 1;       // (only a periodic lattice has a cell in its last column)
    *a = j * D.n_theta + i; *b = *a + 1; *d = jn * D.n_theta + i; *c = *d + 1;
}

__device__ inline double near(double v0, double vk){ return v0 + wrap180(vk - v0); }

// a list segment, decoded from its index: seg = ((m * n_sta + s) * n_planes + p) * n_chunks + chunk, seg < M * n_sta * n_planes * n_chunks
struct Seg { long long m; int s, p, chunk; long long list; };
__device__ inline Seg seg_of(const ListDev& D, long long seg){
    Seg S;
    S.chunk = (int)(seg % D.n_chunks); seg /= D.n_chunks;
    S.p = (int)(seg % D.n_planes); seg /= D.n_planes;
    S.list = seg;                                        // < M * n_sta
    S.s = (int)(seg % D.n_sta); S.m = seg / D.n_sta;
    return S;
}

// the triangle of three corners against a station: all three present, the caller's filter, then the rule of geoac_tri_rule.h
template<class Dev>
__device__ inline Tri tri_test(const Dev& D, const double4& c0, const double4& c1, const double4& c2, double s0, double s1){
    Tri T;
    T.w0 = T.w1 = T.w2 = T.s = 0.0; T.hit = false;
    if(!(c0.w != 0.0 && c1.w != 0.0 && c2.w != 0.0)) return T;
    if(!D.admit(c0, c1, c2)) return T;
    const double x0 = c0.x - s0, x1 = c1.x - s0, x2 = c2.x - s0;
    double y0 = c0.y - s1, y1 = c1.y - s1, y2 = c2.y - s1;
    if(D.spherical){ y0 = wrap180(y0); y1 = wrap180(y1); y2 = wrap180(y2); }
    return tri_rule(x0, y0, x1, y1, x2, y2, D.edge2);
}

// both triangles of the lane's cell on a plane (cell >= cell_end: no hit); plane[r], r < n_rays
template<class Dev>
__device__ inline void cell_test(const Dev& D, const double4* plane, int cell, int cell_end, double s0, double s1, Tri* A, Tri* B, double4* ca, double4* cb,
                                 double4* cc, double4* cd, int* a, int* b, int* c, int* d){
    A->hit = false; B->hit = false;
    if(cell >= cell_end) return;                         // cell < cell_end <= n_cells from here on
    cell_rays(D, cell, a, b, c, d);
    *ca = plane[*a]; *cc = plane[*c];
    if(!(ca->w != 0.0 && cc->w != 0.0)) return;          // (both triangles hold corners a and c)
    *cb = plane[*b]; *cd = plane[*d];
    *A = tri_test(D, *ca, *cb, *cc, s0, s1);
    *B = tri_test(D, *ca, *cc, *cd, s0, s1);
}

// one wave per list segment: its hits
template<class Dev>
__device__ inline void list_count(const Dev& D, long long n_seg_all){
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    for(long long seg = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); seg < n_seg_all; seg += n_waves){
        const Seg S = seg_of(D, seg);
        const double4* plane = D.plane(S);
        const double s0 = D.sta[2 * S.s], s1 = D.sta[2 * S.s + 1];          // s < n_sta
        const int c_begin = S.chunk * LIST_CHUNK;
        const int c_end = c_begin + LIST_CHUNK < D.n_cells ? c_begin + LIST_CHUNK : D.n_cells;
        unsigned n = 0;
        for(int base = c_begin; base < c_end; base += 64){
            Tri A, B; double4 ca, cb, cc, cd; int a, b, c, d;
            cell_test(D, plane, base + lane, c_end, s0, s1, &A, &B, &ca, &cb, &cc, &cd, &a, &b, &c, &d);
            n += (unsigned)__popcll(__ballot(A.hit)) + (unsigned)__popcll(__ballot(B.hit));
        }
        if(lane == 0) D.cnt[S.list * D.nseg + S.p * D.n_chunks + S.chunk] = n;          // [M n_sta][nseg], p * n_chunks + chunk < nseg
    }
}

// one wave per list segment: its base in the list, and its rows
template<class Dev>
__device__ inline void list_rows(const Dev& D, long long n_seg_all){
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    for(long long seg = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); seg < n_seg_all; seg += n_waves){
        const Seg S = seg_of(D, seg);
        const int mine = S.p * D.n_chunks + S.chunk;     // < nseg
        const unsigned* cnt = D.cnt + S.list * D.nseg;
        unsigned before = 0, total = 0;
        for(int k = lane; k < D.nseg; k += 64){          // k < nseg
            const unsigned v = cnt[k];
            total += v;
            before += k < mine ? v : 0u;
        }
        for(int off = 32; off > 0; off >>= 1){
            total += (unsigned)__shfl_xor((int)total, off, 64);
            before += (unsigned)__shfl_xor((int)before, off, 64);
        }
        if(mine == 0 && lane == 0) D.hits[S.list] = total;          // list < M * n_sta
        if(cnt[mine] == 0u || before >= (unsigned)D.cap) continue;
        const double4* plane = D.plane(S);
        const double s0 = D.sta[2 * S.s], s1 = D.sta[2 * S.s + 1];
        const int c_begin = S.chunk * LIST_CHUNK;
        const int c_end = c_begin + LIST_CHUNK < D.n_cells ? c_begin + LIST_CHUNK : D.n_cells;
        const unsigned long long below = (1ull << lane) - 1ull;
        unsigned at = before;
        for(int base = c_begin; base < c_end && at < (unsigned)D.cap; base += 64){
            Tri A, B; double4 ca, cb, cc, cd; int a = 0, b = 0, c = 0, d = 0;
            ca.z = cb.z = cc.z = cd.z = 0.0;
            const int cell = base + lane;
            cell_test(D, plane, cell, c_end, s0, s1, &A, &B, &ca, &cb, &cc, &cd, &a, &b, &c, &d);
            const unsigned long long ma = __ballot(A.hit), mb = __ballot(B.hit);
            const unsigned posA = at + (unsigned)__popcll(ma & below) + (unsigned)__popcll(mb & below);
            const unsigned posB = posA + (A.hit ? 1u : 0u);
            if(A.hit && posA < (unsigned)D.cap)          // row posA < cap of list < M * n_sta
                D.write_row(S, 2 * cell, A, a, b, c, ca, cb, cc, S.list * D.cap + posA);
            if(B.hit && posB < (unsigned)D.cap)
                D.write_row(S, 2 * cell + 1, B, a, c, d, ca, cc, cd, S.list * D.cap + posB);
            at += (unsigned)__popcll(ma) + (unsigned)__popcll(mb);
        }
    }
}

// host half: what both callers keep on the device for their lists, and the steps of a call that they do alike

struct ListBufs {
    void* axes = nullptr; size_t axes_cap = 0;            // theta_ax | phi_ax | sta (| what the caller puts behind them)
    void* cnt = nullptr; size_t cnt_cap = 0;
    void* out = nullptr; size_t out_cap = 0;              // rows | ... | hits
    std::vector<double> h_axes;                           // host copy of what `axes` is filled from (alive while the copy runs)
    EventPair ev;
    void release(){
        if(axes) hipFree(axes);
        if(cnt) hipFree(cnt);
        if(out) hipFree(out);
        ev.release();
    }
};

// the segments of a list, from D->n_cells and the caller's planes; returns the segments of all M * n_sta lists
long long list_segments(ListDev* D, int n_planes){
    D->n_planes = n_planes;
    D->n_chunks = (D->n_cells + LIST_CHUNK - 1) / LIST_CHUNK;
    D->nseg = n_planes * D->n_chunks;
    return (long long)D->M * D->n_sta * D->nseg;
}

// the three buffers: `axes` of axes_tail bytes more than the lattice axes and stations need, `cnt` for n_seg_all segments, `out` of out_need bytes
int list_grow(ListBufs* B, const ListDev& D, size_t axes_tail, long long n_seg_all, size_t out_need){
    const size_t n_axes = (size_t)D.n_theta + D.n_phi + 2 * (size_t)D.n_sta;
    if(grow(&B->axes, &B->axes_cap, sizeof(double) * n_axes + axes_tail) || grow(&B->cnt, &B->cnt_cap, sizeof(unsigned) * (size_t)n_seg_all) ||
       grow(&B->out, &B->out_cap, out_need)) return GEOAC_E_NOMEM;
    return GEOAC_OK;
}

// lattice axes and stations: one host block, one copy (the block lives in the state until the next call).  Returns with the stream idle, so
// a caller may refill a host block of its own behind this; D's pointers into the three buffers are set.
hipError_t list_fill(ListBufs* B, ListDev* D, const GeoacLaunchView& v, const double* sta, hipStream_t s){
    const int nt = D->n_theta, np = D->n_phi;
    const size_t n_axes = (size_t)nt + np + 2 * (size_t)D->n_sta;
    hipError_t e = hipStreamSynchronize(s);               // (an earlier call's copy may still read h_axes)
    if(e != hipSuccess) return e;
    B->h_axes.resize(n_axes);
    for(int i = 0; i < nt; i++) B->h_axes[i] = v.theta_deg[i];
    for(int j = 0; j < np; j++) B->h_axes[nt + j] = v.phi_deg[(size_t)j * nt];
    for(size_t k = 0; k < 2 * (size_t)D->n_sta; k++) B->h_axes[nt + np + k] = sta[k];
    D->theta_ax = (const double*)B->axes; D->phi_ax = D->theta_ax + nt; D->sta = D->phi_ax + np;
    D->cnt = (unsigned*)B->cnt; D->rows = (double*)B->out;
    return hipMemcpyAsync(B->axes, B->h_axes.data(), sizeof(double) * n_axes, hipMemcpyHostToDevice, s);
}

// `out` cleared (a list shorter than cap ends in zero rows), then the two passes
template<class Dev>
hipError_t list_launch(void (*count)(Dev, long long), void (*rows)(Dev, long long), const Dev& D, void* out, size_t out_need, long long n_seg_all, hipStream_t s){
    hipError_t e = hipMemsetAsync(out, 0, out_need, s);
    if(e != hipSuccess || n_seg_all <= 0) return e;
    hipLaunchKernelGGL(count, dim3(blocks_for(n_seg_all, 4)), dim3(256), 0, s, D, n_seg_all);
    hipLaunchKernelGGL(rows, dim3(blocks_for(n_seg_all, 4)), dim3(256), 0, s, D, n_seg_all);
    return hipGetLastError();
}

}  // namespace

#endif
