/* dropest_deflate.h -- BGZF blocks WRITTEN on the device (csrc/k_deflate.h): the compressor under the .rds writer's device switch
 * (csrc/host/facade.h: ResultsPrinter::set_device_compression), behind an interface of its own.
 *
 * The input is cut into chunks of at most 65 280 bytes; every chunk becomes one BGZF block (SAMv1 §4.1): a gzip member (RFC 1952) with the BC
 * field, a raw DEFLATE payload (RFC 1951: one dynamic-Huffman block over LZ77 matches found inside the chunk, or one stored block where that
 * would not be smaller), CRC-32 and ISIZE.  The blocks follow one another densely, so the output is at once a BGZF stream, a sequence of
 * gzip members that zlib's gzread / R's gzfile read as one stream, and -- with the end-of-file block -- the body of a BAM file.  The same
 * input gives the same bytes on every run.  Plain C, no torch types. */
#ifndef DROPEST_DEFLATE_H
#define DROPEST_DEFLATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { DROPEST_DEFLATE_CHUNK = 65280 };
enum { DROPEST_DEFLATE_EOF = 1 };          /* flags bit 0: append the 28-byte BGZF end-of-file block (BAM needs it, .rds does not) */

/* Output bytes that always suffice for `len` input bytes, the end-of-file block included: len + 31 per chunk + 28. */
uint64_t dropest_bgzf_deflate_bound(uint64_t len);
/* Members (BGZF blocks) `len` input bytes become under `flags`: what member_cap must hold. */
uint64_t dropest_bgzf_deflate_members(uint64_t len, int flags);

/* Every pointer is DEVICE memory of `device`.  Asynchronous on `stream` (a hipStream_t, NULL = the default stream); the scratch of the call
 * (about 5 x len) is taken from and given back to the device's stream-ordered pool on the same stream.
 * d_in[0 .. len) is read and nothing else.  d_out[0 .. out_cap) receives the members one after the other, d_member_len[k] the size of member k
 * (member_cap entries: fewer than dropest_bgzf_deflate_members(len, flags) is refused at once), d_totals[0] the number of members, d_totals[1]
 * the bytes of the whole stream, d_totals[2] = 1 when that is more than out_cap: the members that do not fit whole are then NOT written and
 * nothing is written at or beyond d_out + out_cap.  Returns 0, or 1 with dropest_deflate_last_error() set. */
/* WARNING: not beside work on other streams.  With kernels of the same process running on other streams at the same time (the BAM decoder's
 * pipelined windows) and other threads allocating, this call's pool scratch gave blocks of the right size with wrong payload bits (9-22 of 161,
 * different ones every run); the cause was not found.  dropest_deflate_stream_* below makes the same launches with a buffer of its own and
 * did not show it. */
int dropest_bgzf_deflate_device(int device, void *stream, const uint8_t *d_in, uint64_t len, uint8_t *d_out, uint64_t out_cap,
                                uint32_t *d_member_len, uint64_t member_cap, uint64_t *d_totals /* [3] */, int flags);

/* Host buffer in, host buffer out (tests, scripts/bench_deflate.py): upload + the launches of dropest_bgzf_deflate_device (`repeats` times, at
 * least once; *kernel_ms = mean of the runs by HIP events, scratch allocation outside them) + download.  *out_len = bytes of the stream,
 * *n_members = its members.  Returns 0, or 1 with dropest_deflate_last_error() set: no GPU, or out_cap too small -- *out_len then says what is
 * needed and `out` is not touched. */
int dropest_bgzf_deflate_buffer(int device, const uint8_t *data, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                                uint64_t *n_members, double *kernel_ms, int repeats, int flags);

/* ---- batches, host to host, with buffers that stay (the .rds writer's device switch) --------------------------------------------------
 * A handle owns a stream of `device`, pinned host memory for max_bytes of input and dropest_bgzf_deflate_bound(max_bytes) of output, and the
 * device buffers and scratch of one launch of that size (about 7 x max_bytes of device memory in all); _destroy frees all of it.
 * _input: the pinned input buffer, which the caller fills.  _run: its first `len` bytes go up, are deflated by one launch and come back:
 * *out = the stream in the handle's pinned output buffer (valid until the next _run or _destroy), *out_len its bytes.  One thread at a time. */
typedef struct dropest_deflate_batch dropest_deflate_batch;
int dropest_deflate_batch_create(int device, uint64_t max_bytes, dropest_deflate_batch **out);
int dropest_deflate_batch_input(dropest_deflate_batch *b, uint8_t **pinned);
int dropest_deflate_batch_run(dropest_deflate_batch *b, uint64_t len, const uint8_t **out, uint64_t *out_len, uint64_t *n_members);
void dropest_deflate_batch_destroy(dropest_deflate_batch *b);

/* ---- a stream of bytes that are on the device already, to BGZF on the host (the tagged BAM output, -b) ------------------------------------
 * The handle collects what _put gives it in a device buffer of one batch (batch_bytes cut down to whole chunks of 65 280 bytes, at most 64 MB:
 * the scratch of a launch is about 5 x its input, and is the handle's own: dropest_deflate_stream_create's comment in csrc/deflate_api.hip says
 * why it is not the pool's); every full batch is deflated by the launches of dropest_bgzf_deflate_device on `stream` (a hipStream_t of
 * `device` that the caller lends; the copies run there too, so device bytes written on that stream need no other ordering), copied to pinned
 * memory and handed to `write` in order (0 = written).  _put: `src` is DEVICE memory (on_device != 0: copied asynchronously, it must stay as it
 * is until work queued later on the stream runs) or host memory.  _finish deflates what is left over, with `flags` (DROPEST_DEFLATE_EOF: the
 * end-of-file block follows).  Every block but the last of a stream is a full chunk.  _stats: the deflate launches by device events, the bytes
 * deflated and written, the batches so far.  One thread at a time. */
typedef struct dropest_deflate_stream dropest_deflate_stream;
typedef int (*dropest_deflate_write)(const uint8_t *bytes, uint64_t len, void *user);
int dropest_deflate_stream_create(int device, void *stream, uint64_t batch_bytes, dropest_deflate_write write, void *user, dropest_deflate_stream **out);
int dropest_deflate_stream_put(dropest_deflate_stream *s, const uint8_t *src, uint64_t len, int on_device);
int dropest_deflate_stream_finish(dropest_deflate_stream *s, int flags);
int dropest_deflate_stream_stats(const dropest_deflate_stream *s, double *kernel_ms, uint64_t *bytes_in, uint64_t *bytes_out, uint64_t *n_batches);
void dropest_deflate_stream_destroy(dropest_deflate_stream *s);

const char *dropest_deflate_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
