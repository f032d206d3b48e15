// ht_resample_tap.h — the tap of the declared resampler (oracle/canvas_shim.js) on the device, shared by the translation units that
// evaluate it: the pyramid (ht_pyramid.hip) and the video -> canvas draw (ht_ingest.hip).  The host form is ht_host_tap (ht_geometry_plan.h):
// the same binary64 operations in the same order.
#pragma once

#include "ht_internal.h"

typedef HtTap RsTap;  // {t, u: weights of b and a; a, b: source coordinates, absolute incl. the source rect origin}

__device__ __forceinline__ RsTap rs_tap(int i, double r, int s, int origin) {
    double f = __dadd_rn(__dmul_rn((double)i + 0.5, r), -0.5);
    f = f < 0.0 ? 0.0 : f;
    const double fmax = (double)(s - 1);
    f = f > fmax ? fmax : f;
    const double af = floor(f);
    RsTap tp;
    tp.a = origin + (int)af;
    tp.b = origin + min((int)af + 1, s - 1);
    tp.t = __dadd_rn(f, -af);
    tp.u = __dadd_rn(1.0, -tp.t);
    return tp;
}
