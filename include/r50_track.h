/*
 * r50_track.h — C ABI of libr50hip.so, seventh public header: crop + bilinear resize with one box per output frame
 * (INTEGRATION.md section AA).
 *
 * The frame producer of r50.h takes one box and one image size for all frames of a call.  The op here reads both per output frame
 * from a table in device memory, so a crop box can follow the person through a video (`predict --track`) and the frames of a call
 * may differ in size and lie anywhere in one byte buffer.  The conventions are those of r50.h: plain pointers and sizes, 0 on success
 * or a negative r50_status, the text of a refusal through r50_last_error(NULL), every device pointer owned by the caller, the launch
 * on `stream`.  The arithmetic of a frame is the frame producer's, bit for bit, in both modes (R50_RESIZE_FLOAT = 0,
 * R50_RESIZE_FIXED = 1; see r50.h).
 *
 * The table: (t, 9) int64 in device memory, one row per OUTPUT frame:
 *   [0] offset   byte offset of the image's first pixel in src           0 <= offset, offset + 3 H W <= src_bytes
 *   [1] H  [2] W the image at that offset, (H, W, 3) uint8 HWC           H, W >= 1
 *   [3] top  [4] left  [5] hh  [6] ww    the box, inside the image        hh, ww >= 1; ww <= max_ww
 *   [7] px  [8] py   r50_track_weight_precision(ww, out_size) and (hh, out_size); read in fixed mode only, where both are >= 1
 * The kernel trusts the table: the caller checks it on the host (track.BoxTable does) and uploads it.  Rows may repeat, overlap or
 * come in any order: a temporal reverse is a reversed table.
 */
#ifndef R50_TRACK_H_
#define R50_TRACK_H_

#include <stddef.h>
#include <stdint.h>

#ifndef R50_ALIGNED
#define R50_ALIGNED(n)      /* r50.h, "Pointer alignment": the device pointer that follows must be a multiple of n bytes */
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Weight precision (bits) of ATen's native uint8 bilinear resize along one axis of in_size -> out_size: the one definition both frame
 *    ops use in fixed mode.  Host arithmetic, no device.  -1 unless in_size, out_size >= 1. */
int r50_track_weight_precision(int in_size, int out_size);

/* out (t, 3, out_size, out_size) uint8 NCHW: frame i is the box of table row i, resized.  out_flip, if not NULL, receives the same
 *    frames mirrored along the width (`torch.flip(out, dims=[-1])`, the frame producer's R50_AUG_HFLIP output): the four pixels a
 *    thread has computed are stored a second time, to the mirrored quad with their bytes reversed; nothing is read or resampled twice,
 *    and out holds the same bits with and without out_flip.
 *    One launch of t * out_size workgroups of 256, one per (frame, output row).  A workgroup reads its frame's table row (wave-uniform
 *    loads), stages the two source rows of the crop in LDS as dwords from the 4-byte aligned address at or below the crop's first byte
 *    (the misalignment is that of the absolute byte position), reads the last bytes before src + src_bytes byte by byte, and then every
 *    thread produces 4 consecutive pixels of one channel plane.  Dynamic LDS: 2 * ((3 max_ww + 6) & ~3) bytes.
 *    max_ww must be at least every row's ww: the table lives in device memory, so the entry cannot check that, and a row wider than
 *    max_ww would overrun the LDS the launch asked for (track.BoxTable computes max_ww from the rows it checked).
 *    Refused before any launch: src, table or out NULL; src, out or out_flip not 4-byte aligned (the table: 8-byte); out_flip
 *    overlapping out in any byte; src_bytes < 1;
 *    t < 1; out_size < 4, > 4096 or not a multiple of 4; an unknown mode; max_ww < 1 or LDS beyond 160 KB; t * out_size >= 2^31.
 *    Asynchronous on `stream`, no host read, no allocation, no atomics: the same bits on every run. */
int r50_op_crop_resize_boxes_u8(const void* R50_ALIGNED(4) src_u8, int64_t src_bytes, const int64_t* table_dev, int t, int max_ww,
                                void* R50_ALIGNED(4) out_tchw_u8, void* R50_ALIGNED(4) out_flip_tchw_u8, int out_size, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_TRACK_H_ */
