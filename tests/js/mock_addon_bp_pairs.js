'use strict';
/* tests/js/mock_addon_bp_pairs.js — TEST INFRASTRUCTURE: tests/js/mock_addon_pairs.js (left as it is) plus camshiftBackProjectPairs of
 * csrc/ht_napi.cc, computed on the host from the oracle state's model histogram (the first 4096 uint32 of ho_cs_state) with the
 * reference's formulas (camshift.js:49-72, 314-353, 177-196), so that camshift.MultiTracker's getBackProjectionImg(i) /
 * getBackProjectionImgs() / getPdf(i) and ccv.DeviceBatch.backProjectionPairs run without a GPU.  The pair-list rules are those of the
 * other pair calls.  `withBpPairs(false)` removes the entry point again: an addon that lacks it, for the facade's host-loop path. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_pairs.js'));

function count(name) { mock.calls[name] = (mock.calls[name] || 0) + 1; }
function live(c) { if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context'); return c; }
function frameOf(c, f) { return c.frames.subarray(f * c.stride, f * c.stride + c.w * c.h * 4); }
function bin(d, p) { return 256 * (d[p] >> 4) + 16 * (d[p + 1] >> 4) + (d[p + 2] >> 4); }

function checkPairs(c, pairs) {
  if (!(pairs instanceof Int32Array) || pairs.length < 2 || (pairs.length & 1)) throw new TypeError('mock addon: camshiftBackProjectPairs(ctx, Int32Array pairs[2n], kind)');
  const n = pairs.length >> 1, seen = {};
  if (n > c.cs.length) throw new Error('mock addon: status -1: more pairs than reserved streams');
  if (!c.frames || c.n < 1) throw new Error('mock addon: status -6: bind frames first');
  for (let i = 0; i < n; i++) {
    const s = pairs[2 * i], f = pairs[2 * i + 1];
    if (s < 0 || s >= c.cs.length) throw new Error('mock addon: status -1: stream ' + s + ' is not reserved');
    if (f < 0 || f >= c.n) throw new Error('mock addon: status -1: frame ' + f + ' is not bound');
    if (seen[s]) throw new Error('mock addon: status -1: stream ' + s + ' appears twice');
    seen[s] = true;
  }
  return n;
}

const bpFns = {
  camshiftBackProjectPairs: function (c, pairs, kind) {
    count('camshiftBackProjectPairs'); live(c);
    if (arguments.length < 3) throw new TypeError('mock addon: camshiftBackProjectPairs(ctx, Int32Array pairs[2n], kind)');
    const n = checkPairs(c, pairs);
    if (kind !== mock.BP_RGBA8 && kind !== mock.BP_F64) throw new TypeError('mock addon: camshiftBackProjectPairs: kind = BP_RGBA8 | BP_F64');
    const npix = c.w * c.h;
    const out = kind === mock.BP_F64 ? new Float64Array(n * npix) : new Uint8Array(4 * n * npix);
    const hists = {}; /* the frame's histogram once per distinct frame */
    for (let i = 0; i < n; i++) {
      const st = c.cs[pairs[2 * i]], f = pairs[2 * i + 1], d = frameOf(c, f);
      if (!hists[f]) {
        const h = new Uint32Array(4096);
        for (let p = 0; p < 4 * npix; p += 4) h[bin(d, p)]++;
        hists[f] = h;
      }
      const cur = hists[f], model = st ? new Uint32Array(st.buffer, st.byteOffset, 4096) : new Uint32Array(4096); /* never initialised: zeros */
      const w = new Float64Array(4096);
      for (let b = 0; b < 4096; b++) w[b] = cur[b] !== 0 ? Math.min(model[b] / cur[b], 1) : 0;
      for (let q = 0; q < npix; q++) {
        const v = w[bin(d, 4 * q)];
        if (kind === mock.BP_F64) out[i * npix + q] = v;
        else { const o = 4 * (i * npix + q), g = Math.floor(255 * v); out[o] = g; out[o + 1] = g; out[o + 2] = g; out[o + 3] = 255; }
      }
    }
    return out;
  }
};

if (mock.BP_RGBA8 === undefined) { mock.BP_RGBA8 = 0; mock.BP_F64 = 1; }
mock.withBpPairs = function (on) {
  Object.keys(bpFns).forEach(function (k) { if (on) mock[k] = bpFns[k]; else delete mock[k]; });
  return mock;
};
mock.withBpPairs(true);
module.exports = mock;
