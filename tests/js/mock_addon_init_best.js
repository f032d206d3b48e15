'use strict';
/* tests/js/mock_addon_init_best.js — TEST INFRASTRUCTURE: tests/js/mock_addon_group.js (left as it is) plus the two entry points of the
 * record-driven initTracker of csrc/ht_napi.cc — camshiftInitBest, camshiftInitBestResult — on the CPU oracle, so that the host logic of
 * new ccv.DeviceBatch(.., {grouping: 'device', handoff: 'device'}) runs without a GPU.  The call-sequence rules are those of
 * ht_camshift_init_best(_result): a device-grouped batch must be in flight, or collected and not yet overwritten (status -6 otherwise);
 * the pair-list rules of the pair calls, a frame below the grouped batch's frame count and a threshold that is not NaN (status -1), all
 * checked before anything changes; the result belongs to the LAST call, with the same n, until camshiftReserve grows the reservation.
 * The decision is facetrackr.js:97-107 on the oracle's best face; the mock has no grouping cap, so no pair is ever deferred.
 * `withInitBest(false)` is an addon that lacks the calls. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_group.js'));
const oracle = require(path.join(__dirname, 'oracle_addon.node'));

mock.CSB_UNTOUCHED = 0; mock.CSB_FACE = 1; mock.CSB_FALLBACK = 2; mock.CSB_DEFERRED = 3;
function count(name) { mock.calls[name] = (mock.calls[name] || 0) + 1; }
function live(c) { if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context'); return c; }

/* the records the device holds: of the batch in flight when a grouping is enqueued behind it, else of the batch collected last */
function records(c) {
  const e = c.enqueued;
  if (e && e.best) {
    const best = new Float64Array(6 * e.n);
    for (let f = 0; f < e.n; f++)
      best.set(oracle.bestFace(e.frames.subarray(f * e.stride, f * e.stride + c.w * c.h * 4), c.w, c.h, e.flags & 1, c.cascade, c.interval, e.best.mn).subarray(0, 6), 6 * f);
    return { n: e.n, best: best };
  }
  if (c.grouped && c.grouped.lists !== false) return { n: c.grouped.n, best: c.grouped.best };
  throw new Error('mock addon: status -6: no device-grouped batch');
}

const fns = {
  camshiftInitBest: function (c, pairs, minConfidence, fallback) {
    count('camshiftInitBest'); live(c);
    const usage = 'mock addon: camshiftInitBest(ctx, Int32Array pairs[2n], minConfidence, Int32Array fallback[4n] | null)';
    if (!(pairs instanceof Int32Array) || pairs.length < 2 || (pairs.length & 1) || typeof minConfidence !== 'number') throw new TypeError(usage);
    const n = pairs.length >> 1, seen = {};
    if (fallback !== undefined && fallback !== null && (!(fallback instanceof Int32Array) || fallback.length < 4 * n)) throw new TypeError(usage);
    const rec = records(c);
    if (minConfidence !== minConfidence) throw new Error('mock addon: status -1: min_confidence is NaN');
    if (n > c.cs.length) throw new Error('mock addon: status -1: more pairs than reserved streams');
    if (!c.frames || c.n < 1) throw new Error('mock addon: status -6: bind frames first');
    for (let i = 0; i < n; i++) {
      const s = pairs[2 * i], f = pairs[2 * i + 1];
      if (s < 0 || s >= c.cs.length) throw new Error('mock addon: status -1: stream ' + s + ' is not reserved');
      if (f < 0 || f >= c.n) throw new Error('mock addon: status -1: frame ' + f + ' is not bound');
      if (f >= rec.n) throw new Error('mock addon: status -1: frame ' + f + ' is outside the device-grouped batch');
      if (seen[s]) throw new Error('mock addon: status -1: stream ' + s + ' appears twice');
      seen[s] = true;
    }
    const codes = new Int32Array(n), rects = new Int32Array(4 * n);
    for (let i = 0; i < n; i++) {
      const s = pairs[2 * i], f = pairs[2 * i + 1], b = rec.best.subarray(6 * f, 6 * f + 6);
      if (b[5] > 0 && b[4] > minConfidence) { codes[i] = mock.CSB_FACE; for (let k = 0; k < 4; k++) rects[4 * i + k] = Math.floor(b[k]); }
      else if (fallback) { codes[i] = mock.CSB_FALLBACK; rects.set(fallback.subarray(4 * i, 4 * i + 4), 4 * i); }
      else continue; /* untouched */
      const st = new Uint8Array(oracle.csStateBytes);
      oracle.csInit(st, c.frames.subarray(f * c.stride, f * c.stride + c.w * c.h * 4), c.w, c.h, rects[4 * i], rects[4 * i + 1], rects[4 * i + 2], rects[4 * i + 3], 1);
      c.cs[s] = st;
    }
    c.csb = { n: n, codes: codes, rects: rects, reserved: c.cs.length };
  },
  camshiftInitBestResult: function (c, n) {
    count('camshiftInitBestResult'); live(c);
    if (typeof n !== 'number' || n !== (n | 0) || n <= 0) throw new TypeError('mock addon: camshiftInitBestResult(ctx, n)');
    if (!c.csb) throw new Error('mock addon: status -6: no camshiftInitBest to report on');
    if (c.csb.reserved !== c.cs.length) throw new Error('mock addon: status -6: camshiftReserve has replaced the trackers since');
    if (c.csb.n !== n) throw new Error('mock addon: status -6: n differs from the last camshiftInitBest');
    return { codes: Int32Array.from(c.csb.codes), rects: Int32Array.from(c.csb.rects) };
  }
};

mock.withInitBest = function (on) {
  Object.keys(fns).forEach(function (k) { if (on) mock[k] = fns[k]; else delete mock[k]; });
  return mock;
};
mock.withInitBest(true);
module.exports = mock;
