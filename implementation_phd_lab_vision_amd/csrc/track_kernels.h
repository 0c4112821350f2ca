// Crop + bilinear resize with one box per output frame (include/r50_track.h, INTEGRATION.md section AA).
// Included after kernels.h: resize_taps, resize_stage_row and resize_quad are the ones crop_resize_u8_kernel uses, so a frame holds the
// bits the frame producer gives for the same image and box.
#pragma once

#define TRACK_COLS 9      // offset, H, W, top, left, hh, ww, px, py

struct TrackArgs {
    const unsigned char* src;       // the byte buffer the table's offsets refer to, 4-byte aligned
    long long src_bytes;
    const long long* table;         // (T, TRACK_COLS), checked by the caller
    unsigned char* dst;             // (T, 3, out, out)
    unsigned char* dst_flip;        // the same mirrored along the width, or nullptr
    int out;
    int float_mode;
};

// One workgroup = one output row of one frame, as in crop_resize_u8_kernel; box, image size and precisions come from the frame's table
// row (uniform over the workgroup: scalar loads).  The LDS rows are as wide as this frame's crop; the launch sizes LDS for the widest.
__global__ __launch_bounds__(256) void crop_resize_boxes_u8_kernel(const TrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
    const int quads = a.out >> 2;
    const int t = blockIdx.x / a.out, yo = blockIdx.x - t * a.out;
    const long long* row = a.table + (size_t)t * TRACK_COLS;
    const size_t off = (size_t)row[0];
    const int W = (int)row[2], top = (int)row[3], left = (int)row[4], hh = (int)row[5], ww = (int)row[6];
    const int px = (int)row[7], py = (int)row[8];
    const bool fm = a.float_mode != 0;
    int y0, wy0, wy1;
    resize_taps(yo, hh, a.out, py, fm, y0, wy0, wy1);
    const int y1 = min(y0 + 1, hh - 1);
    // absolute byte positions of the crop's first byte in the two source rows
    const size_t g0 = off + ((size_t)(top + y0) * W + left) * 3, g1 = off + ((size_t)(top + y1) * W + left) * 3;
    const int row_bytes = ww * 3;
    const int row_pad = (row_bytes + 3 + 3) & ~3;                     // room for the leading misalignment
    // copy [g & ~3, g + row_bytes) of both rows as dwords; sh = g & 3 is where the crop starts inside the copy (src is 4-byte aligned)
    const int sh0 = (int)(g0 & 3), sh1 = (int)(g1 & 3);
    const unsigned* s0 = reinterpret_cast<const unsigned*>(a.src + (g0 - sh0));
    const unsigned* s1 = reinterpret_cast<const unsigned*>(a.src + (g1 - sh1));
    const int nd0 = (sh0 + row_bytes + 3) >> 2, nd1 = (sh1 + row_bytes + 3) >> 2;
    unsigned* l0 = reinterpret_cast<unsigned*>(tk_smem);
    unsigned* l1 = reinterpret_cast<unsigned*>(tk_smem + row_pad);
    const unsigned char* src_end = a.src + a.src_bytes;
    resize_stage_row(s0, nd0, src_end, l0);
    resize_stage_row(s1, nd1, src_end, l1);
    __syncthreads();
    const unsigned char* row0 = tk_smem + sh0;
    const unsigned char* row1 = tk_smem + row_pad + sh1;
    const size_t plane = (size_t)a.out * a.out;
    for (int item = threadIdx.x; item < quads * 3; item += 256) {
        const int c = item / quads, xq = item - c * quads;
        const unsigned packed = resize_quad(row0, row1, xq, c, ww, a.out, px, py, fm, false, wy0, wy1);
        const size_t at = ((size_t)t * 3 + c) * plane + (size_t)yo * a.out;
        *reinterpret_cast<unsigned*>(a.dst + at + xq * 4) = packed;
        // torch.flip(.., dims=[-1]): column x of the mirrored frame is column out - 1 - x, so this quad lands in quad quads - 1 - xq
        // with its four bytes in reverse order
        if (a.dst_flip) *reinterpret_cast<unsigned*>(a.dst_flip + at + (quads - 1 - xq) * 4) = __builtin_bswap32(packed);
    }
}
