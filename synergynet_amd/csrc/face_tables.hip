// Detector output -> crop kernel input without the host (syn_compact_detections, syn_face_tables, syn_lanczos4_tables): the
// vis_thres filter of FaceBoxes.__call__ (FaceBoxes.py:131-141) over the padded rows of syn_detect_batch, the ROI / box arithmetic of
// get_all_outputs (synergy3DMM.py:178-185) and the Lanczos-4 tap tables of synergynet_amd/inference.py, per face.  The arithmetic
// itself is face_tables.h (shared with a host harness); nothing here is near a roof of the chip -- a call is a few microseconds of
// a handful of workgroups -- so the kernels are plain: one workgroup per face, one lane per destination index.
#include "syn_internal.h"
#include "face_tables.h"

namespace syn {

// grid n, 128 lanes: lane dx < 120 owns destination index dx of sides[i]
__global__ __launch_bounds__(128) void lanczos4_tables_kernel(const int *__restrict__ sides, int *__restrict__ ofs /*[n,120]*/,
                                                              short *__restrict__ coef /*[n,120,8]*/) {
    const int i = blockIdx.x, dx = threadIdx.x;
    if (dx >= kFtDst) return;
    int side = sides[i];
    side = side < 1 ? 1 : side;                       // (the entry point refuses such a call; never index by it anyway)
    int o;
    int16_t c[8];
    ft_lanczos4_tap(side, dx, &o, c);
    const size_t at = (size_t)i * kFtDst + dx;
    ofs[at] = o;
#pragma unroll
    for (int k = 0; k < 8; ++k) coef[at * 8 + k] = c[k];
}

// grid n, 256 lanes: every lane restates the face's box (five broadcast loads), lanes 0..119 own the x index, 120..239 the y index
__global__ __launch_bounds__(256) void face_tables_kernel(const float *__restrict__ dets /*[n,5]*/, float *__restrict__ roi /*[n,5]*/,
                                                          int *__restrict__ box /*[n,4]*/, int *__restrict__ xofs, short *__restrict__ xcoef,
                                                          int *__restrict__ yofs, short *__restrict__ ycoef, int *__restrict__ status) {
    const int i = blockIdx.x, t = threadIdx.x;
    if (t >= 2 * kFtDst) return;
    float d[5], r[5];
    int b[4], w, h;
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = dets[(size_t)i * 5 + k];
    const int st = ft_roi_box(d, r, b, &w, &h);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) roi[(size_t)i * 5 + k] = r[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) box[(size_t)i * 4 + k] = b[k];
        status[i] = st;
    }
    const bool is_y = t >= kFtDst;
    const int dx = is_y ? t - kFtDst : t;
    int o;
    int16_t c[8];
    ft_lanczos4_tap(is_y ? h : w, dx, &o, c);
    const size_t at = (size_t)i * kFtDst + dx;
    (is_y ? yofs : xofs)[at] = o;
    short *cd = (is_y ? ycoef : xcoef) + at * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) cd[k] = c[k];
}

// ONE workgroup of 4 waves; wave v owns output frames v, v + 4, ...  Pass 1 counts each frame's rows with score > thres among its
// first min(max(count, 0), K) rows (rows past the count are uninitialised memory and are never read) into frame_faces[i]; pass 2 gives
// every wave its frame's base = sum of the counts before it (the exclusive scan, each wave for itself) and copies the rows in order.
__global__ __launch_bounds__(256) void compact_detections_kernel(const float *__restrict__ dets /*[N,K,5]*/, const int *__restrict__ counts,
                                                                 const int *__restrict__ order /*nullable*/, int N, int K, float thres,
                                                                 float *__restrict__ rows, int *__restrict__ face_frame,
                                                                 int *__restrict__ frame_faces /*[N+1]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < N; i += 4) {
        const int src = order ? order[i] : i;
        int c = 0;
        if (src >= 0 && src < N) c = min(max(counts[src], 0), K);      // an index outside the batch is a frame without faces
        int found = 0;
        for (int j0 = 0; j0 < c; j0 += 64) {
            const int j = j0 + lane;
            const bool ok = j < c && dets[((size_t)src * K + j) * 5 + 4] > thres;      // strict; NaN is not greater
            found += __popcll(__ballot(ok));
        }
        if (lane == 0) frame_faces[i] = found;
    }
    __syncthreads();                                   // (workgroup-scope fence: the counts are visible to every wave)
    if (threadIdx.x == 0) {
        int total = 0;
        for (int i = 0; i < N; ++i) total += frame_faces[i];
        frame_faces[N] = total;
    }
    for (int i = wave; i < N; i += 4) {
        int base = 0;
        for (int j = lane; j < i; j += 64) base += frame_faces[j];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) base += __shfl_xor(base, m, 64);
        const int src = order ? order[i] : i;
        int c = 0;
        if (src >= 0 && src < N) c = min(max(counts[src], 0), K);
        for (int j0 = 0; j0 < c; j0 += 64) {
            const int j = j0 + lane;
            const float *row = dets + ((size_t)src * K + (j < c ? j : 0)) * 5;
            const bool ok = j < c && row[4] > thres;
            const unsigned long long mask = __ballot(ok);
            if (ok) {
                const size_t at = (size_t)base + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
                for (int k = 0; k < 5; ++k) rows[at * 5 + k] = row[k];
                face_frame[at] = i;
            }
            base += __popcll(mask);
        }
    }
}

void launch_lanczos4_tables(const int *sides, int n, int *ofs, short *coef, hipStream_t s) {
    lanczos4_tables_kernel<<<n, 128, 0, s>>>(sides, ofs, coef);
}

void launch_face_tables(const float *dets, int n, float *roi, int *box, int *xofs, short *xcoef, int *yofs, short *ycoef, int *status,
                        hipStream_t s) {
    face_tables_kernel<<<n, 256, 0, s>>>(dets, roi, box, xofs, xcoef, yofs, ycoef, status);
}

void launch_compact_detections(const float *dets, const int *counts, const int *order, int N, int K, float thres, float *rows,
                               int *face_frame, int *frame_faces, hipStream_t s) {
    compact_detections_kernel<<<1, 256, 0, s>>>(dets, counts, order, N, K, thres, rows, face_frame, frame_faces);
}

}  // namespace syn
