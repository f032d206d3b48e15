'use strict';
/* tests/js/mock_addon_pairs.js — TEST INFRASTRUCTURE: tests/js/mock_addon.js (left as it is) plus the pair entry points of csrc/ht_napi.cc —
 * camshiftInitPairs, camshiftTrackPairs — on the CPU oracle, so that the host logic of ccv.DeviceBatch's initPairs / trackPairs /
 * trackPairsEnqueue / detectStepFinish(.., {feeds}) and of camshift.MultiTracker runs without a GPU.  The argument rules are those of
 * ht_camshift_*_pairs: checked before anything changes, status -1 (HT_ERR_INVALID) / -6 (HT_ERR_STATE) in the message.  Enqueue-only
 * steps share the plain mock's ring (c.ring) with camshiftTrackBound's.  `withPairs(false)` is the plain mock: an addon that lacks the
 * calls, for the facade's error path. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon.js'));
const oracle = require(path.join(__dirname, 'oracle_addon.node'));

const CS_CALC_ANGLES_OFFSET = 4096 * 4 + 4 * 4 + 5 * 8; /* ho_cs_state.calc_angles */
const TRACK_RING = 4;
function count(name) { mock.calls[name] = (mock.calls[name] || 0) + 1; }
function live(c) { if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context'); return c; }
function frameOf(c, f) { return c.frames.subarray(f * c.stride, f * c.stride + c.w * c.h * 4); }

function checkPairs(c, what, pairs) {
  if (!(pairs instanceof Int32Array) || pairs.length < 2 || (pairs.length & 1)) throw new TypeError('mock addon: ' + what + '(ctx, Int32Array pairs[2n], ...)');
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

const pairFns = {
  camshiftInitPairs: function (c, pairs, rects) {
    count('camshiftInitPairs'); live(c);
    const n = checkPairs(c, 'camshiftInitPairs', pairs);
    if (!(rects instanceof Int32Array) || rects.length < 4 * n) throw new TypeError('mock addon: camshiftInitPairs(ctx, Int32Array pairs[2n], Int32Array rects[4n])');
    for (let i = 0; i < n; i++) {
      const st = new Uint8Array(oracle.csStateBytes);
      oracle.csInit(st, frameOf(c, pairs[2 * i + 1]), c.w, c.h, rects[4 * i], rects[4 * i + 1], rects[4 * i + 2], rects[4 * i + 3], 1);
      c.cs[pairs[2 * i]] = st;
    }
  },
  camshiftTrackPairs: function (c, pairs, calcAngles, fetch) {
    count('camshiftTrackPairs'); live(c);
    const n = checkPairs(c, 'camshiftTrackPairs', pairs);
    for (let i = 0; i < n; i++) if (!c.cs[pairs[2 * i]]) throw new Error('mock addon: track on a slot without initTracker');
    if (fetch === false && c.ring.length >= TRACK_RING) throw new Error('mock addon: status -6: more than ' + TRACK_RING + ' enqueue-only track steps outstanding');
    const out = new Float64Array(9 * n);
    for (let i = 0; i < n; i++) {
      const st = c.cs[pairs[2 * i]];
      new DataView(st.buffer).setInt32(CS_CALC_ANGLES_OFFSET, calcAngles ? 1 : 0, true);
      out.set(oracle.csTrack(st, frameOf(c, pairs[2 * i + 1]), c.w, c.h), 9 * i);
    }
    if (fetch !== false) return out;
    c.ring.push(out);
    return undefined;
  }
};

mock.withPairs = function (on) {
  Object.keys(pairFns).forEach(function (k) { if (on) mock[k] = pairFns[k]; else delete mock[k]; });
  return mock;
};
mock.withPairs(true);
module.exports = mock;
