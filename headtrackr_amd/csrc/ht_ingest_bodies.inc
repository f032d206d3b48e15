// ht_ingest_bodies.inc — the text of the draw kernels' tile, written once and compiled by every kernel that draws: k_draw_frames
// (ht_ingest.hip), k_draw_yuv<NV12 | I420> (ht_ingest_yuv.hip), k_draw_list (ht_draw_list.hip), which holds all three pixel bodies behind one
// workgroup-uniform branch, and through ht_list_parts.inc's scaffold the face-patch kernels and k_draw_list_mean_tile (ht_draw_filter.hip).
// Included INSIDE a kernel, with IG_BODY_PART naming the piece:
//
//   IG_BODY_TAPS   X0, Y0 and the tile's 64 column and 16 row taps into s_col / s_row (the kernel declares the arrays and places the barrier)
//   IG_BODY_RGBA   the RGBA pixel body, behind the barrier
//   IG_BODY_YUV    the NV12 / I420 / YUYV / UYVY pixel body, behind the barrier; FMT is the template parameter, a constant of the enclosing
//                  scope or — where one inclusion serves several formats (k_draw_list_mean_tile alone: I420 and the packed 4:2:2,
//                  LP_PACKED_422) — the entry's format, a workgroup-uniform value.  With a constant NV12 / I420 the packed branches fold away
//
// The text reads the names the single-source kernels give their parameters — src, src_pitch, src_stride (RGBA); yp, up, vp, y_pitch,
// c_pitch, stride, cw, kc (YUV; 4:2:2 reads yp, y_pitch, stride, cw, kc: cw is then the row's macropixel count); dst, dst_stride, sx,
// sy, sw, sh, dw, dh, rx, ry — and k_draw_list binds the same names to its entry's descriptor before it includes a piece (frame strides
// 0: an entry is one frame).
//
// Shared as TEXT on purpose, as ht_cs_kernels.inc is.  The same bodies as __device__ __forceinline__ functions called from thin kernels
// compile to other machine code: the extra inlining level reorders the optimiser's passes, and k_draw_frames went from 50 to 74 VGPRs —
// over the 64 that tests/test_ingest_cpu.py holds it to (8 wavefronts per SIMD).  Included as text, k_draw_frames and k_draw_yuv<> are the
// instructions they were.
//
// Each piece begins with IG_NEEDS lines: the names it reads from the enclosing scope and the type each must convert to.  A kernel that
// renames a parameter, or binds a name to something of another kind, stops compiling here instead of rebinding the text silently.
#ifndef IG_NEEDS
#define IG_NEEDS(name, type) static_assert(std::is_convertible<decltype(name), type>::value && sizeof(name) == sizeof(type), "ht_ingest_bodies.inc needs " #name " as " #type)
#endif
// The pixel bodies end in ONE output stage, IG_STORE(o, x, y): o is the pixel's RGBA8 dword, (x, y) its place in the destination.  The default
// is the dword store into `out` (the destination's base + x) that every draw kernel and k_crop_list take; a kernel with another output
// stage (ht_patch.hip: the model-input tensors) defines IG_STORE before it includes a piece and puts the default back behind itself.
#define IG_STORE_DWORD(o, x, y) out[(size_t)(y) * dw] = (o)
#ifndef IG_STORE
#define IG_STORE IG_STORE_DWORD
#endif
#define IG_BODY_TAPS 1
#define IG_BODY_RGBA 2
#define IG_BODY_YUV 3

#if IG_BODY_PART == IG_BODY_TAPS
    IG_NEEDS(sx, int); IG_NEEDS(sy, int); IG_NEEDS(sw, int); IG_NEEDS(sh, int); IG_NEEDS(dw, int); IG_NEEDS(dh, int); IG_NEEDS(rx, double); IG_NEEDS(ry, double);
    IG_NEEDS(&s_col[0], RsTap *); IG_NEEDS(&s_row[0], RsTap *);
    const int X0 = blockIdx.x * IG_TW, Y0 = blockIdx.y * IG_TH;
    if (threadIdx.x < IG_TW) s_col[threadIdx.x] = rs_tap(min(X0 + (int)threadIdx.x, dw - 1), rx, sw, sx);
    else if (threadIdx.x < IG_TW + IG_TH) s_row[threadIdx.x - IG_TW] = rs_tap(min(Y0 + (int)threadIdx.x - IG_TW, dh - 1), ry, sh, sy);

#elif IG_BODY_PART == IG_BODY_RGBA
    IG_NEEDS(src, const uint8_t *); IG_NEEDS(src_pitch, size_t); IG_NEEDS(src_stride, size_t); IG_NEEDS(dst, uint8_t *); IG_NEEDS(dst_stride, size_t);
    IG_NEEDS(sx, int); IG_NEEDS(sw, int); IG_NEEDS(dw, int); IG_NEEDS(dh, int); IG_NEEDS(X0, int); IG_NEEDS(Y0, int);
    const int col = threadIdx.x & (IG_TW - 1), r0 = threadIdx.x / IG_TW, x = X0 + col;
    if (x >= dw) return;
    const RsTap cx = s_col[col];
    // the tap pair (a, b) as ONE 8-byte read: b == a + 1 unless a is the rect's last column (then b == a and the pair is read one
    // pixel to the left, both taps taking its right half); a 1-pixel-wide rect has no pair and is read pixel by pixel
    const bool pair = sw >= 2;
    const int xa = pair ? min(cx.a, sx + sw - 2) : cx.a;
    const bool right = cx.a != xa;
    const uint8_t *frame = src + (size_t)blockIdx.z * src_stride + (size_t)xa * 4;
    ig_u32x2 top2[IG_RPT], bot2[IG_RPT];
    double ru[IG_RPT], rt[IG_RPT];
    bool on[IG_RPT];
#pragma unroll
    for (int k = 0; k < IG_RPT; k++) {
        const int j = r0 + k * (IG_NT / IG_TW);
        on[k] = Y0 + j < dh;
        const RsTap ty = s_row[j];
        ru[k] = ty.u, rt[k] = ty.t;
        top2[k] = bot2[k] = ig_u32x2{0u, 0u};
        if (on[k]) {
            const uint8_t *pa = frame + (size_t)ty.a * src_pitch, *pb = frame + (size_t)ty.b * src_pitch;
            if (pair) {
                top2[k] = *reinterpret_cast<const ig_u32x2 *>(pa);
                bot2[k] = *reinterpret_cast<const ig_u32x2 *>(pb);
            } else {
                top2[k].x = top2[k].y = *reinterpret_cast<const uint32_t *>(pa);
                bot2[k].x = bot2[k].y = *reinterpret_cast<const uint32_t *>(pb);
            }
        }
    }
    uint32_t *out = reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.z * dst_stride) + x;
#pragma unroll
    for (int k = 0; k < IG_RPT; k++) {
        if (!on[k]) continue;
        const uint32_t p00 = right ? top2[k].y : top2[k].x, p01 = top2[k].y, p10 = right ? bot2[k].y : bot2[k].x, p11 = bot2[k].y;
        uint32_t o = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) o |= ig_channel(p00, p01, p10, p11, 8 * ch, cx.u, cx.t, ru[k], rt[k]);
        IG_STORE(o, x, Y0 + r0 + k * (IG_NT / IG_TW));
    }

#elif IG_BODY_PART == IG_BODY_YUV
    IG_NEEDS(yp, const uint8_t *); IG_NEEDS(up, const uint8_t *); IG_NEEDS(vp, const uint8_t *); IG_NEEDS(y_pitch, size_t); IG_NEEDS(c_pitch, size_t); IG_NEEDS(stride, size_t);
    IG_NEEDS(dst, uint8_t *); IG_NEEDS(dst_stride, size_t); IG_NEEDS(sx, int); IG_NEEDS(sw, int); IG_NEEDS(cw, int); IG_NEEDS(dw, int); IG_NEEDS(dh, int);
    IG_NEEDS(X0, int); IG_NEEDS(Y0, int); IG_NEEDS(kc, HtYuvCoef); IG_NEEDS(FMT, int);
    const int col = threadIdx.x & (IG_TW - 1), r0 = threadIdx.x / IG_TW, x = X0 + col;
    if (x >= dw) return;
    const RsTap cx = s_col[col];
    // packed 4:2:2 (YUYV / UYVY): ONE plane (yp, y_pitch) of 4-byte macropixels, cw of them per row; up, vp and c_pitch are not read
    const bool packed = ht_yuv_is_422(FMT);
    const bool pair = sw >= 2;
    const int xa = pair ? min(cx.a, sx + sw - 2) : cx.a;  // the Y pair's anchor, inside the rect
    const int ya_sel = cx.a - xa, yb_sel = cx.b - xa;      // 0 / 1: which byte of the pair each tap takes
    const bool cpair = cw >= 2;
    // the chroma pair's anchor, inside the frame's chroma row.  4:2:2: the MACROPIXEL pair's — the tap pair (a, b), b == a or a + 1, names
    // at most two adjacent macropixels, (a >> 1) and (a >> 1) + 1, and a row holds cw whole ones whatever the rect is
    const int ca = cpair ? min(cx.a >> 1, cw - 2) : 0;
    const int ca_sel = (cx.a >> 1) - ca, cb_sel = (cx.b >> 1) - ca;
    // a macropixel as a dword, low byte first: YUYV Y0 U Y1 V, UYVY U Y0 V Y1
    const int ush = FMT == HT_YUV_FMT_UYVY ? 0 : 8, ma_sh = 8 - ush + 16 * (cx.a & 1), mb_sh = 8 - ush + 16 * (cx.b & 1);
    const size_t foff = (size_t)blockIdx.z * stride;
    const uint8_t *yf = yp + foff + (packed ? (size_t)ca * 4 : (size_t)xa), *uf = up + foff, *vf = FMT == HT_YUV_FMT_NV12 ? uf : vp + foff;
    uint32_t ytop[IG_RPT], ybot[IG_RPT], ctop[IG_RPT], cbot[IG_RPT];  // 4:2:2: macropixel 0 of the pair in y.., macropixel 1 in c..
    double ru[IG_RPT], rt[IG_RPT];
    bool on[IG_RPT];
    // (the format is tested ONCE around each row loop, not per row: where it is a run-time value the planar loop stays the straight-line
    // code it is with a constant format, all its reads in front of the first use)
    if (packed) {
#pragma unroll
        for (int k = 0; k < IG_RPT; k++) {
            const int j = r0 + k * (IG_NT / IG_TW);
            on[k] = Y0 + j < dh;
            const RsTap ty = s_row[j];
            ru[k] = ty.u, rt[k] = ty.t;
            ytop[k] = ybot[k] = ctop[k] = cbot[k] = 0u;
            if (on[k]) {
                // ONE 8-byte read per row at a 4-byte-aligned address (the plan requires base and pitch to be multiples of 4), the form the
                // RGBA body reads its pixel pair in; a frame of 1 or 2 pixels' width has one macropixel and is read as a single dword
                const uint8_t *pa = yf + (size_t)ty.a * y_pitch, *pb = yf + (size_t)ty.b * y_pitch;
                if (cpair) {
                    const ig_u32x2 t2 = *reinterpret_cast<const ig_u32x2 *>(pa), b2 = *reinterpret_cast<const ig_u32x2 *>(pb);
                    ytop[k] = t2.x, ctop[k] = t2.y, ybot[k] = b2.x, cbot[k] = b2.y;
                } else {
                    ytop[k] = ctop[k] = *reinterpret_cast<const uint32_t *>(pa);
                    ybot[k] = cbot[k] = *reinterpret_cast<const uint32_t *>(pb);
                }
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < IG_RPT; k++) {
            const int j = r0 + k * (IG_NT / IG_TW);
            on[k] = Y0 + j < dh;
            const RsTap ty = s_row[j];
            ru[k] = ty.u, rt[k] = ty.t;
            ytop[k] = ybot[k] = ctop[k] = cbot[k] = 0u;
            if (on[k]) {
                const uint8_t *pa = yf + (size_t)ty.a * y_pitch, *pb = yf + (size_t)ty.b * y_pitch;
                if (pair) {
                    ytop[k] = *reinterpret_cast<const ig_u16b *>(pa);
                    ybot[k] = *reinterpret_cast<const ig_u16b *>(pb);
                } else {
                    ytop[k] = *pa;
                    ybot[k] = *pb;
                }
                ctop[k] = ig_chroma_read(FMT, uf, vf, (size_t)(ty.a >> 1) * (FMT == HT_YUV_FMT_NV12 ? c_pitch / 2 : c_pitch) + (size_t)ca, cpair);
                cbot[k] = ig_chroma_read(FMT, uf, vf, (size_t)(ty.b >> 1) * (FMT == HT_YUV_FMT_NV12 ? c_pitch / 2 : c_pitch) + (size_t)ca, cpair);
            }
        }
    }
    uint32_t *out = reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.z * dst_stride) + x;
#pragma unroll
    for (int k = 0; k < IG_RPT; k++) {
        if (!on[k]) continue;
        // the four tap pixels as the RGBA8 dwords k_draw_frames would have read
        uint32_t p00, p01, p10, p11;
        if (packed) {  // each tap's macropixel, then Y, U and V by shifts out of the lane's registers
            // (selected by a per-lane mask word, 0 or ~0, not by a lane-mask register pair: the list kernels with a tensor output are short of SGPRs)
            const uint32_t am = 0u - (uint32_t)ca_sel, bm = 0u - (uint32_t)cb_sel, tx = ytop[k] ^ ctop[k], bx = ybot[k] ^ cbot[k];
            const uint32_t ta = ytop[k] ^ (tx & am), tb = ytop[k] ^ (tx & bm), ba = ybot[k] ^ (bx & am), bb = ybot[k] ^ (bx & bm);
            p00 = ht_yuv_to_rgba((ta >> ma_sh) & 0xffu, (ta >> ush) & 0xffu, (ta >> ush >> 16) & 0xffu, kc);
            p01 = ht_yuv_to_rgba((tb >> mb_sh) & 0xffu, (tb >> ush) & 0xffu, (tb >> ush >> 16) & 0xffu, kc);
            p10 = ht_yuv_to_rgba((ba >> ma_sh) & 0xffu, (ba >> ush) & 0xffu, (ba >> ush >> 16) & 0xffu, kc);
            p11 = ht_yuv_to_rgba((bb >> mb_sh) & 0xffu, (bb >> ush) & 0xffu, (bb >> ush >> 16) & 0xffu, kc);
        } else {
            const uint32_t ta = ctop[k] >> (16 * ca_sel), tb = ctop[k] >> (16 * cb_sel), ba = cbot[k] >> (16 * ca_sel), bb = cbot[k] >> (16 * cb_sel);
            p00 = ht_yuv_to_rgba((ytop[k] >> (8 * ya_sel)) & 0xffu, ta & 0xffu, (ta >> 8) & 0xffu, kc);
            p01 = ht_yuv_to_rgba((ytop[k] >> (8 * yb_sel)) & 0xffu, tb & 0xffu, (tb >> 8) & 0xffu, kc);
            p10 = ht_yuv_to_rgba((ybot[k] >> (8 * ya_sel)) & 0xffu, ba & 0xffu, (ba >> 8) & 0xffu, kc);
            p11 = ht_yuv_to_rgba((ybot[k] >> (8 * yb_sel)) & 0xffu, bb & 0xffu, (bb >> 8) & 0xffu, kc);
        }
        uint32_t o = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) o |= ig_channel(p00, p01, p10, p11, 8 * ch, cx.u, cx.t, ru[k], rt[k]);
        IG_STORE(o, x, Y0 + r0 + k * (IG_NT / IG_TW));
    }

#else
#error "IG_BODY_PART names no piece"
#endif
#undef IG_BODY_PART
