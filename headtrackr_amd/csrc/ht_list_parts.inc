// ht_list_parts.inc — the text the face-patch kernels share, written once: k_crop_list (ht_crop.hip), k_align_list (ht_align.hip),
// k_cut_tensor<> / k_upright_tensor<> (ht_patch.hip), k_cut_mean<> / k_upright_mean<> (ht_filter.hip).  Included INSIDE a kernel, with
// LP_PART naming the piece:
//
//   LP_CUT_HEAD       the head of a cut kernel: the entry's descriptor and its stream's state (scalar loads), the crop rule and the record
//                     (workgroup (0, 0)).  Leaves e, d, format, stream, rc, code, (sx, sy, sw, sh) = the rule's rect and rx, ry = the
//                     record's ratios, the unfiltered patch's sw / dw, sh / dh (a kernel whose taps have other ratios defines
//                     LP_RATIOS_OF_RECORD_ONLY in front: the two then exist inside the record's branch alone)
//   LP_UPRIGHT_HEAD   the head of an upright kernel: the same with the align rule.  Leaves e, d, format, stream, SW, SH, pl, code
//                     Behind either head the kernel makes its output stage where it needs it and takes the empty exit, uniformly and in
//                     front of the barrier: if (code != HT_CROP_FACE) return lp_empty_tile<IG_RPT>(store, dw, dh)  (ht_crop.hip)
//   LP_UPRIGHT_TERMS  X0, Y0 and the unfiltered patch's Q16 terms of the tile's 64 columns and 16 rows into s_cx, s_cy / s_rx, s_ry: the
//                     column terms carry the centre and the pixel-centre offset, so a pixel adds its row's term and is done (the kernel
//                     declares the arrays and places the barrier)
//   LP_SCAFFOLD       behind the barrier: the workgroup-uniform branch on the entry's format into the three pixel bodies of
//                     ht_ingest_bodies.inc, their parameter names bound to the entry's descriptor d (frame strides 0: an entry is one
//                     frame).  LP_EACH_PASS, when the kernel defines it, stands in front of each body's block — statement heads that end
//                     where a block may follow (ht_filter.hip: the loops over the fine patch's slices and, as an if's initialiser, the
//                     slice's s_col / s_row); it is undefined again behind the scaffold.  LP_PACKED_422, when the kernel defines it (as a constant expression that is true), makes the
//                     third body take the packed 4:2:2 formats (YUYV, UYVY) besides I420 (ht_draw_filter.hip: the one kernel every draw of
//                     a packed source goes through); without it a kernel is the instructions it was, and its host path hands it no such entry (the
//                     face-patch calls unpack a packed entry's frame to RGBA first: dm_unpack_sources, ht_draw_calls.hip)
//
// The including kernel binds: tab, states, recs, dw, dh, cw_canvas, ch_canvas, margin_q8, flags (its parameters; dst and dst_stride for the
// bodies), and the tile through IG_TW / IG_TH / IG_RPT / IG_NT as the pixel bodies read them (a kernel with another tile declares
// constants of those names in its own scope).
//
// Shared as TEXT, as ht_ingest_bodies.inc and ht_cs_kernels.inc are and for their reason: the pieces as __forceinline__ functions called
// from thin kernels compile to other machine code.  Each piece begins with LP_NEEDS lines: the names it reads from the enclosing scope and
// the type each must convert to, so that a kernel that renames a parameter stops compiling here.
#ifndef LP_NEEDS
#define LP_NEEDS(name, type) static_assert(std::is_convertible<decltype(name), type>::value && sizeof(name) == sizeof(type), "ht_list_parts.inc needs " #name " as " #type)
#endif
#define LP_CUT_HEAD 1
#define LP_UPRIGHT_HEAD 2
#define LP_UPRIGHT_TERMS 3
#define LP_SCAFFOLD 4

#if LP_PART == LP_CUT_HEAD || LP_PART == LP_UPRIGHT_HEAD
    LP_NEEDS(tab, const CrDesc *); LP_NEEDS(states, const HtCsState *); LP_NEEDS(dw, int); LP_NEEDS(dh, int); LP_NEEDS(cw_canvas, int); LP_NEEDS(ch_canvas, int);
    LP_NEEDS(margin_q8, int); LP_NEEDS(flags, uint32_t);
    const CrDesc &e = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const DlDesc &d = e.d;
#if LP_PART == LP_CUT_HEAD
    LP_NEEDS(recs, ht_crop_record *);
    const int format = d.format, stream = e.stream;
    const HtCsState &st = states[stream];
    ht_cs_rect rc;
    const int32_t code = ht_crop_rule(st.x, st.y, st.width, st.height, cw_canvas, ch_canvas, e.SW, e.SH, d.sx, d.sy, d.sw, d.sh, margin_q8, flags, &rc);
    const int sx = rc.x, sy = rc.y, sw = rc.width, sh = rc.height;
    // one correctly rounded binary64 division each: the bits of the host's (double)sw / (double)dw
#define LP_RATIOS const double rx = code == HT_CROP_FACE ? (double)sw / (double)dw : 0.0, ry = code == HT_CROP_FACE ? (double)sh / (double)dh : 0.0
#ifndef LP_RATIOS_OF_RECORD_ONLY
    LP_RATIOS;  // the record's and the taps'
#endif
    if ((blockIdx.x | blockIdx.y) == 0 && threadIdx.x == 0) {
#ifdef LP_RATIOS_OF_RECORD_ONLY
        LP_RATIOS;  // divided by the one thread that writes them
#undef LP_RATIOS_OF_RECORD_ONLY
#endif
#undef LP_RATIOS
        ht_crop_record r;
        r.code = code, r.stream = stream, r.rect = rc, r.rx = rx, r.ry = ry;
        recs[blockIdx.z] = r;
    }
#else
    LP_NEEDS(recs, ht_align_record *);
    const int format = d.format, stream = e.stream, SW = e.SW, SH = e.SH;
    const HtCsState &st = states[stream];
    HtAlignPlan pl;
    const int32_t code = ht_align_rule(st.x, st.y, st.width, st.height, st.angle, cw_canvas, ch_canvas, SW, SH, d.sx, d.sy, d.sw, d.sh, margin_q8, flags, &pl);
    if ((blockIdx.x | blockIdx.y) == 0 && threadIdx.x == 0) {
        ht_align_record r;
        r.code = code, r.stream = stream, r.a12 = pl.a12, r.pad = 0;
        r.cx = pl.cx, r.cy = pl.cy, r.ux = pl.ux, r.uy = pl.uy, r.vx = pl.vx, r.vy = pl.vy;
        recs[blockIdx.z] = r;
    }
#endif

#elif LP_PART == LP_UPRIGHT_TERMS
    LP_NEEDS(pl, HtAlignPlan); LP_NEEDS(dw, int); LP_NEEDS(dh, int);
    LP_NEEDS(&s_cx[0], int64_t *); LP_NEEDS(&s_cy[0], int64_t *); LP_NEEDS(&s_rx[0], int64_t *); LP_NEEDS(&s_ry[0], int64_t *);
    const int X0 = blockIdx.x * IG_TW, Y0 = blockIdx.y * IG_TH;
    if (threadIdx.x < IG_TW) {
        const int i = min(X0 + (int)threadIdx.x, dw - 1);
        s_cx[threadIdx.x] = pl.cx - 32768 + ht_align_term(i, dw, pl.ux);
        s_cy[threadIdx.x] = pl.cy - 32768 + ht_align_term(i, dw, pl.uy);
    } else if (threadIdx.x < IG_TW + IG_TH) {
        const int j = min(Y0 + (int)threadIdx.x - IG_TW, dh - 1);
        s_rx[threadIdx.x - IG_TW] = ht_align_term(j, dh, pl.vx);
        s_ry[threadIdx.x - IG_TW] = ht_align_term(j, dh, pl.vy);
    }

#elif LP_PART == LP_SCAFFOLD
    LP_NEEDS(d, DlDesc); LP_NEEDS(format, int);
#ifndef LP_EACH_PASS
#define LP_EACH_PASS
#endif
    if (format == HT_DRAW_RGBA) {
        const uint8_t *__restrict__ src = (const uint8_t *)d.p0;
        const size_t src_pitch = d.pitch0, src_stride = 0;
        LP_EACH_PASS {
#define IG_BODY_PART 2  // IG_BODY_RGBA
#include "ht_ingest_bodies.inc"
        }
    } else {
        const uint8_t *__restrict__ yp = (const uint8_t *)d.p0, *__restrict__ up = (const uint8_t *)d.p1, *__restrict__ vp = (const uint8_t *)d.p2;
        const size_t y_pitch = d.pitch0, c_pitch = d.pitch1, stride = 0;
        const int cw = d.cw;
        const HtYuvCoef kc = d.kc;
        if (format == HT_YUV_FMT_NV12) {
            constexpr int FMT = HT_YUV_FMT_NV12;
            LP_EACH_PASS {
#define IG_BODY_PART 3  // IG_BODY_YUV
#include "ht_ingest_bodies.inc"
            }
        } else {
#ifdef LP_PACKED_422  // (a constant expression of the kernel) I420, YUYV or UYVY in this ONE inclusion and ONE compiled body: the format is a
            // workgroup-uniform value in it; where the expression is false FMT folds to the constant and the kernel is the instructions it was
            const int FMT = (LP_PACKED_422) ? format : HT_YUV_FMT_I420;
#else
            constexpr int FMT = HT_YUV_FMT_I420;
#endif
            LP_EACH_PASS {
#define IG_BODY_PART 3  // IG_BODY_YUV
#include "ht_ingest_bodies.inc"
            }
        }
    }
#undef LP_EACH_PASS
#undef LP_PACKED_422

#else
#error "LP_PART names no piece"
#endif
#undef LP_PART
