// orbx_describe.h -- orientation + rotated BRIEF-256 of ONE keypoint by one wavefront (describe_wave) with the LDS
// working set and the job record it takes: shared by k_describe_flat (orbx_kernels.hip) and k_pd_describe
// (orbx_reloc.hip).  Device code, gfx950 only.  The including file defines c_pattern, the 256 test pairs of
// pattern_31.inc as 1024 int8_t in constant memory (16-byte aligned), and includes orbx_math.h and orbx_wave.h first.
#pragma once
#define DESC_R 20
#define DESC_ROWS (2 * DESC_R + 1)  // 41
#define DESC_PITCH 48               // bytes per LDS patch row (12 dwords)
#define DESC_HP 40                  // u16 entries per row of the box-sum tables
#define DESC_BROWS (DESC_ROWS - 4)  // 37 rows of 5x5 box sums

// per-wavefront LDS working set
struct DescLds {
  // the patch is dead once the horizontal sums exist, so the 5x5 table reuses its
  // space (6.2 KB per wave -> 6 workgroups per CU instead of 4)
  union {
    uint32_t patch[DESC_ROWS * DESC_PITCH / 4];  // 41 x 48 u8
    uint16_t box[DESC_BROWS * DESC_HP];          // 5x5 sums: box[r][j] = sum hs[r..r+4][j]
  };
  uint16_t hs[DESC_ROWS * DESC_HP];  // horizontal 5-sums: hs[r][j] = sum patch[r][j..j+4]
};

// the four 5-byte sums b[k..k+4], k = 0..3, of the 8 bytes (d0 low), as packed u16.
// v_qsad_pk_u16_u8 against 0 gives the four sliding 4-byte sums b[k..k+3] plus a packed
// accumulator, which carries b[k+4]: one instruction instead of ~20 byte extracts and adds.
__device__ __forceinline__ u64 hsum5x4(uint32_t d0, uint32_t d1) {
  const u64 acc = (u64)__builtin_amdgcn_perm(d1, d1, 0x0c010c00u) |
                  ((u64)__builtin_amdgcn_perm(d1, d1, 0x0c030c02u) << 32);
  return __builtin_amdgcn_qsad_pk_u16_u8((u64)d0 | ((u64)d1 << 32), 0u, acc);
}

struct DescJob {
  const uint8_t* img;
  int w, h, pitch;
  int x, y;
  bool valid;
};

// The 512 box sums a descriptor needs are looked up in a per-keypoint table of
// ALL 5x5 box sums of the 41x41 neighbourhood, built with two separable passes
// of wide, conflict-free LDS accesses (2 dword reads -> 4 sums -> one 8-byte
// write; 5 8-byte reads -> one 8-byte write) instead of 25 scattered byte reads
// per sample.  Sums are exact integers (<= 6375), identical to what the
// reference derives from its integral image (src/orb_cpu.cpp:190-201).
__device__ __forceinline__ void describe_wave(const DescJob& jb, DescLds& lds, int patch_size,
                                              bool use_given_angle, float given_angle, bool do_brief,
                                              float& angle_out, u64 desc_out[4]) {
  const int lane = lane_id();
  const uint8_t* s_patch = reinterpret_cast<const uint8_t*>(lds.patch);
  const int px0 = jb.x - DESC_R, py0 = jb.y - DESC_R;
  const int ax0 = px0 & ~3;  // floor to a multiple of 4 (two's complement)
  const int off = px0 - ax0;
  if (jb.valid) {
    // item i = lane + 64k -> (row, dword column); 64 = 5 * 12 + 4 gives the increments
    int row = lane / (DESC_PITCH / 4), c = lane - row * (DESC_PITCH / 4);
#pragma unroll
    for (int k = 0; k < (DESC_ROWS * (DESC_PITCH / 4) + 63) / 64; k++) {
      const int i = lane + 64 * k;
      if (i < DESC_ROWS * (DESC_PITCH / 4)) {
        const int gy = py0 + row, gx = ax0 + 4 * c;
        uint32_t v = 0;
        // gx, pitch are multiples of 4: (unsigned)gx < pitch  <=>  0 <= gx && gx + 4 <= pitch
        if ((unsigned)gy < (unsigned)jb.h && (unsigned)gx < (unsigned)jb.pitch)
          v = *reinterpret_cast<const uint32_t*>(jb.img + (uint32_t)(gy * jb.pitch + gx));
        lds.patch[i] = v;
      }
      row += 5;
      c += 4;
      if (c >= DESC_PITCH / 4) {
        c -= DESC_PITCH / 4;
        row += 1;
      }
    }
  }
  __syncthreads();
  float angle = 0.0f;
  if (jb.valid) {
    if (use_given_angle) {
      angle = given_angle;
    } else {
      const int pr = patch_size / 2, P = 2 * pr + 1;
      // full patch must lie inside the image, else 0 (src/orb_cpu.cpp:152-156)
      if (!(jb.x - pr < 0 || jb.x + pr >= jb.w || jb.y - pr < 0 || jb.y + pr >= jb.h)) {
        // lanes = patch columns (two row groups when the patch is <= 32 wide),
        // rows in the loop: no per-pixel division, one LDS byte read per step
        const int grp_shift = P <= 32 ? 5 : 6;
        const int col = lane & ((1 << grp_shift) - 1), grp = lane >> grp_shift, ngrp = 64 >> grp_shift;
        int colsum = 0, m01 = 0;
        if (col < P) {
          const uint8_t* pc = s_patch + (DESC_R - pr) * DESC_PITCH + (col - pr + DESC_R + off);
          for (int rr = grp; rr < P; rr += ngrp) {
            const int I = pc[rr * DESC_PITCH];
            colsum += I;
            m01 += (rr - pr) * I;
          }
        }
        int m10 = (col - pr) * colsum;
        m10 = wave_sum(m10);
        m01 = wave_sum(m01);
        // the reference accumulates in float; every partial sum is an integer
        // below 2^24, hence exact, hence equal to this int32 sum
        angle = orbx_atan2f((float)m01, (float)m10);
      }
    }
  }
  angle_out = angle;
  if (!do_brief) return;

  // pass 1: horizontal 5-sums, 4 per item (row r, dword group g); item i = lane + 64k,
  // 64 = 6 * 10 + 4 gives the increments
  if (jb.valid) {
    int r = lane / 10, g = lane - r * 10;
#pragma unroll
    for (int k = 0; k < (DESC_ROWS * 10 + 63) / 64; k++) {
      if (lane + 64 * k < DESC_ROWS * 10) {
        const uint32_t d0 = lds.patch[r * (DESC_PITCH / 4) + g], d1 = lds.patch[r * (DESC_PITCH / 4) + g + 1];
        *reinterpret_cast<u64*>(&lds.hs[r * DESC_HP + 4 * g]) = hsum5x4(d0, d1);
      }
      r += 6;
      g += 4;
      if (g >= 10) {
        g -= 10;
        r += 1;
      }
    }
  }
  __syncthreads();
  // pass 2: vertical 5-sums of the horizontal sums
  if (jb.valid) {
    int r = lane / 10, g = lane - r * 10;
#pragma unroll
    for (int k = 0; k < (DESC_BROWS * 10 + 63) / 64; k++) {
      if (lane + 64 * k < DESC_BROWS * 10) {
        const uint2* hp = reinterpret_cast<const uint2*>(&lds.hs[r * DESC_HP + 4 * g]);
        uint2 acc = hp[0];
#pragma unroll
        for (int q = 1; q < 5; q++) {
          const uint2 v = hp[q * (DESC_HP / 4)];
          acc.x = pk_add(acc.x, v.x);
          acc.y = pk_add(acc.y, v.y);
        }
        *reinterpret_cast<uint2*>(&lds.box[r * DESC_HP + 4 * g]) = acc;
      }
      r += 6;
      g += 4;
      if (g >= 10) {
        g -= 10;
        r += 1;
      }
    }
  }
  __syncthreads();

  const float c = orbx_cosf(angle), s = orbx_sinf(angle);
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    bool bit = false;
    if (jb.valid) {
      const int i = k * 64 + lane;
      const int32_t pk = reinterpret_cast<const int32_t*>(c_pattern)[i];
      const float x1 = (float)(int8_t)(pk & 0xff), y1 = (float)(int8_t)((pk >> 8) & 0xff);
      const float x2 = (float)(int8_t)((pk >> 16) & 0xff), y2 = (float)(int8_t)((pk >> 24) & 0xff);
      // lround(c*x - s*y), lround(s*x + c*y): separate IEEE mul / add-sub,
      // round half away from zero (src/orb_cpu.cpp:228-232)
      int dx1 = orbx_lroundf(__fsub_rn(__fmul_rn(c, x1), __fmul_rn(s, y1)));
      int dy1 = orbx_lroundf(__fadd_rn(__fmul_rn(s, x1), __fmul_rn(c, y1)));
      int dx2 = orbx_lroundf(__fsub_rn(__fmul_rn(c, x2), __fmul_rn(s, y2)));
      int dy2 = orbx_lroundf(__fadd_rn(__fmul_rn(s, x2), __fmul_rn(c, y2)));
      const int cx1 = jb.x + dx1, cy1 = jb.y + dy1, cx2 = jb.x + dx2, cy2 = jb.y + dy2;
      // bounds check of the reference, in image terms: integral width-2 ==
      // cols-1 (src/orb_cpu.cpp:240-245)
      const bool skip = cx1 < 2 || cy1 < 2 || cx1 > jb.w - 1 || cy1 > jb.h - 1 || cx2 < 2 || cy2 < 2 ||
                        cx2 > jb.w - 1 || cy2 > jb.h - 1;
      if (!skip) {
        // memory safety for angles outside the documented domain
        dx1 = min(max(dx1, -18), 18);
        dy1 = min(max(dy1, -18), 18);
        dx2 = min(max(dx2, -18), 18);
        dy2 = min(max(dy2, -18), 18);
        const int s1 = lds.box[(dy1 + 18) * DESC_HP + dx1 + 18 + off];
        const int s2 = lds.box[(dy2 + 18) * DESC_HP + dx2 + 18 + off];
        bit = s1 < s2;
      }
    }
    desc_out[k] = __ballot(bit);
  }
}
