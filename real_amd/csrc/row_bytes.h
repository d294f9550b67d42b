// row_bytes.h -- where the bytes of a simple bucket row lie in a lane's transposed LDS copy.  No HIP in here (as
// row_addr.h): tests/test_row_bytes_cpu.py compiles it with the host compiler and compares it with rh_row_entry_hw and the
// dword swizzle it replaces.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define RH_HD __host__ __device__
#else
#define RH_HD
#endif

// A row is 128 bytes: eight pieces of 16.  The transpose of the paired driver stores piece p of the row of lane L at piece
// p ^ (L & 7) of the lane's 128 bytes (no bank conflicts on either side), so row byte B lies at byte B ^ ((L & 7) << 4).
static inline RH_HD uint32_t rh_row_lds_byte(uint32_t B, uint32_t sw) { return B ^ (sw << 4); }
// Entry j of a simple row (6 bytes from byte 8 on): the u16 key at byte 8 + 6 j, the u32 position in the four bytes behind it,
// low half first.  All three halfwords are 2-byte aligned, so none of them crosses a piece -- the position as a whole does
// for entries 6 and 14 (bytes 46 .. 49, 94 .. 97) and is therefore read as two halves.
static inline RH_HD uint32_t rh_row_key_byte(uint32_t j) { return 8u + 6u * j; }
static inline RH_HD uint32_t rh_row_pos_byte(uint32_t j, uint32_t half) { return 10u + 6u * j + 2u * half; }
