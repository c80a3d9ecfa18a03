// The key-point half of data/sequence_dataloader.py:105-198 on pseudo labels that are resident in HBM (kpx_amd/resident.py): what
// SequenceDataLoader.render does to the key points with numpy -- gather 33 sets (or 17 and the means of neighbours), rotate, flip, scale,
// one-hot action code -- restated operation for operation in the precision numpy uses there, so that every float32 equals the host's.
//
//   gap >= 1   the gathered array is float32 and stays float32: the Python-float constants are rounded to float32 first.
//   gap == 0   the mean of two neighbours is a float32 add and divide; it lands in a float64 array, the rotation, flip and scale are float64
//              operations with the double constants, and the result is rounded to float32 once (the collate's astype).
//
// Cosine, sine and the scale are computed on the host (math.cos / math.sin / randint / 100.0) and reach the kernel as doubles: no
// transcendental and no division by anything but two runs here.  Every product and sum rounds once (seq_*: no fma).  One thread per point.
#include "kpx_common.h"

enum { S_VIDEO = 0, S_IM_IDX, S_GAP, S_FLAGS, S_ANGLE, S_SCALE_LO, S_SCALE_HI, S_ACTION };

template <typename T> __device__ __forceinline__ T seq_mul(T a, T b) {
#pragma clang fp contract(off)
    return a * b;
}
template <typename T> __device__ __forceinline__ T seq_add(T a, T b) {
#pragma clang fp contract(off)
    return a + b;
}
template <typename T> __device__ __forceinline__ T seq_sub(T a, T b) {
#pragma clang fp contract(off)
    return a - b;
}

// utils/data.py:63-72 about the origin, then the flip (:177-180) and the scale (:186-187), in T: qx = 0 + c*x - s*y, qy = 0 + s*x + c*y, summed
// left to right; the added 0 turns a -0.0 product into +0.0 as it does on the host.
template <typename T> __device__ __forceinline__ void seq_transform(T& x, T& y, int flags, double c, double s, double scale) {
    if (flags & KPX_SEQ_ROTATE) {
        const T ct = (T)c, st = (T)s;
        const T qx = seq_sub(seq_add((T)0, seq_mul(ct, x)), seq_mul(st, y));
        const T qy = seq_add(seq_add((T)0, seq_mul(st, x)), seq_mul(ct, y));
        x = qx; y = qy;
    }
    if (flags & KPX_SEQ_FLIP) x = seq_mul(x, (T)-1);
    if (flags & KPX_SEQ_SCALE) { x = seq_mul(x, (T)scale); y = seq_mul(y, (T)scale); }
}

__global__ __launch_bounds__(256) void keypoint_seq_augment_kernel(const float* __restrict__ labels, const int64_t* __restrict__ label_off,
                                                                   const int32_t* __restrict__ rows, int n_rows, int K, int n_action,
                                                                   const double* __restrict__ trig, float* __restrict__ keypoints,
                                                                   float* __restrict__ real_seq, float* __restrict__ action_code) {
    const int per_row = KPX_SEQ_LEN * K + n_action;              // the points of the 33 sets, then the action code's entries
    const int id = blockIdx.x * 256 + threadIdx.x;               // n_rows * per_row < 2^31 (the entry's bounds)
    if (id >= n_rows * per_row) return;
    const int n = id / per_row, j = id - n * per_row;
    const int32_t* row = rows + (size_t)n * KPX_SEQ_ROW_INTS;
    if (j >= KPX_SEQ_LEN * K) {
        const int a = j - KPX_SEQ_LEN * K;
        action_code[(size_t)n * n_action + a] = a == row[S_ACTION] ? 1.0f : 0.0f;
        return;
    }
    const int t = j / K, k = j - t * K;
    const int im_idx = row[S_IM_IDX], gap = row[S_GAP], flags = row[S_FLAGS];
    const float* src = labels + label_off[row[S_VIDEO]] + (size_t)k * 2;
    const double c = trig[row[S_ANGLE] * 2], s = trig[row[S_ANGLE] * 2 + 1];
    const double scale = __hiloint2double(row[S_SCALE_HI], row[S_SCALE_LO]);
    float ox, oy;
    if (gap >= 1) {
        const float* p = src + (size_t)(im_idx + gap * t) * K * 2;
        ox = p[0]; oy = p[1];
        seq_transform<float>(ox, oy, flags, c, s, scale);
    } else {
        const float* p = src + (size_t)(im_idx + (t >> 1)) * K * 2;
        float hx = p[0], hy = p[1];
        if (t & 1) {                                             // (half[i] + half[i + 1]) / 2.0 in float32; halving rounds as the division does
            const float* q = p + (size_t)K * 2;
            hx = seq_mul(seq_add(hx, q[0]), 0.5f);
            hy = seq_mul(seq_add(hy, q[1]), 0.5f);
        }
        double dx = (double)hx, dy = (double)hy;
        seq_transform<double>(dx, dy, flags, c, s, scale);
        ox = (float)dx; oy = (float)dy;
    }
    float* dst = t == 0 ? keypoints + ((size_t)n * K + k) * 2 : real_seq + (((size_t)n * (KPX_SEQ_LEN - 1) + (t - 1)) * K + k) * 2;
    dst[0] = ox; dst[1] = oy;
}

extern "C" int kpx_keypoint_seq_augment_f32(const float* labels, const int64_t* label_off, const int32_t* rows, int n_rows, int n_points,
                                            int n_action, const double* trig, float* keypoints, float* real_seq, float* action_code,
                                            void* stream) {
    if (!labels || !label_off || !rows || !trig || !keypoints || !real_seq || !action_code) return KPX_EINVAL;
    if (n_rows < 0 || n_rows > KPX_SEQ_MAX_ROWS || n_points < 1 || n_points > KPX_SEQ_MAX_POINTS || n_action < 1 || n_action > KPX_SEQ_MAX_ACTIONS)
        return KPX_EINVAL;
    if (n_rows == 0) return 0;
    const int total = n_rows * (KPX_SEQ_LEN * n_points + n_action);          // <= 4096 * (33 * 256 + 256) < 2^27
    hipLaunchKernelGGL(keypoint_seq_augment_kernel, dim3((total + 255) / 256), dim3(256), 0, kpx_stream(stream),
                       labels, label_off, rows, n_rows, n_points, n_action, trig, keypoints, real_seq, action_code);
    return kpx_launch_status();
}
