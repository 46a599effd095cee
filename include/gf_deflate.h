/* gf_deflate — text deflated on the device into BGZF members: C ABI of libgfdeflate.so.
 *
 * The counterpart of gf_inflate.h: what libgfwrite.so formats (gf_read_write.h) leaves the device compressed, as a file
 * that bgzip, htslib and gf_if_inflate_device read member by member.
 *
 * The format.  The text is cut into members of GF_DF_TEXT_BYTES = 65280 bytes of text, bgzip's size, the last one
 * shorter; text of 0 bytes gives no member.  Each member is a BGZF member exactly as gf_inflate.h defines one:
 *     the 18-byte header  1f 8b 08 04 00000000 00 ff 0600 'B' 'C' 0200 BSIZE-1 (the member's size - 1, 16 bits)
 *     one raw DEFLATE stream of ONE final block: LZ77 tokens under dynamic Huffman codes, or stored when that is not
 *     longer
 *     CRC-32 and ISIZE of the text, 32 bits each.
 * A stored member is GF_DF_STORED_BYTES_OVER = 31 bytes longer than its text, so every member fits 64 KiB.  A file
 * ends with the 28-byte BGZF end-of-file marker (GF_DF_EOF_MARKER), which is the caller's to write, once.
 *
 * Which bytes the encoder chooses is no contract; that they are a function of the member's text alone is: the same text
 * gives the same member on every run, on the device and in gf_df_member_host.  The choices are stated once, in
 * genefuserust_amd/scan_csrc/gf_df_core.h, as code both sides compile.
 *
 * What may be READ around the text: the kernels load the text in aligned 16-byte pieces, so up to 15 bytes in front of
 * d_text and up to 15 bytes behind d_text + text_cap, inside the aligned pieces that hold the first and the last byte
 * (never another page: an allocation's own granule).  Nothing outside d_out[0, out_cap), d_member_off[0, members] and
 * the workspace is written.
 *
 * No gf_index is taken: the device is that of the pointers.  The library is built next to libgfmatch.so and links
 * against it like its siblings, but calls nothing of it on the device.  Conventions are those of gfmatch.h: plain
 * pointers and sizes, caller owns every buffer, GF_OK or a negative GF_ERR_* code, with a message for the calling thread
 * in gf_df_last_error().
 */
#ifndef GF_DEFLATE_H
#define GF_DEFLATE_H

#include "gfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF_DF_TEXT_BYTES 65280   /* text bytes per member */
#define GF_DF_STORED_BYTES_OVER 31 /* header 18 + stored block header 5 + trailer 8 */
#define GF_DF_TOTALS 5           /* int64 per d_totals */
#define GF_DF_EOF_MARKER_BYTES 28
#define GF_DF_EOF_MARKER "\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0"

/* Members that text_cap bytes of text make at most: ceil(text_cap / 65280).  0 for text_cap <= 0. */
int64_t gf_df_members(int64_t text_cap);

/* Bytes d_out needs for them: text_cap + 31 * gf_df_members(text_cap). */
int64_t gf_df_out_cap(int64_t text_cap);

/* Device bytes gf_df_deflate_device needs as d_workspace: per member a 64 KiB slot, 2 * 65280 bytes of tokens and its
 * size, and 256 bytes to align the caller's base.  All three functions are non-decreasing in text_cap. */
int64_t gf_df_workspace_bytes(int64_t text_cap);

/* The text deflated, one asynchronous call queued on `stream` (a hipStream_t, NULL = default stream): no allocation, no
 * host synchronisation and no copy between host and device.  Every pointer is device memory on the device of d_out
 * (GF_ERR_NO_DEVICE when it is not device memory: there is no CPU fallback).
 *   d_text: uint8[text_cap], any alignment (see above for what is read around it).  text_cap sizes the grid.
 *   d_text_bytes: int64 on the device, the true length of the text, read by the kernels (values outside [0, text_cap]
 *   are cut to it); NULL: text_cap.  Members past the true length write nothing and count as absent.
 *   d_out: uint8[out_cap], out_cap >= gf_df_out_cap(text_cap): the members back to back, d_member_off[members] bytes.
 *   d_member_off: int64[gf_df_members(text_cap) + 1]: where each member starts; an absent member starts where the output
 *   ends.
 *   d_totals: int64[GF_DF_TOTALS], ADDED into: [0] members, [1] bytes of text, [2] compressed bytes, [3] members stored,
 *   [4] members under dynamic codes.
 *   GF_ERR_CAPACITY for a short out_cap or workspace, before anything is launched. */
int gf_df_deflate_device(const void* d_text, int64_t text_cap, const void* d_text_bytes, void* d_out, int64_t out_cap,
                         void* d_member_off, void* d_totals, void* d_workspace, int64_t workspace_bytes, void* stream);

/* Host code, no GPU: the member the device writes for text[0, n), 1 <= n <= 65280, byte for byte, into out[0, out_cap);
 * *out_bytes: its size.  GF_ERR_CAPACITY when out_cap is less than that (n + 31 always suffices), GF_ERR_ARG for n
 * outside the range. */
int gf_df_member_host(const void* text, int64_t n, void* out, int64_t out_cap, int64_t* out_bytes);

/* The message of the calling thread's last failed gf_df_* call. */
const char* gf_df_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GF_DEFLATE_H */
