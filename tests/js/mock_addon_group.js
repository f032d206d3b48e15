'use strict';
/* tests/js/mock_addon_group.js — TEST INFRASTRUCTURE: tests/js/mock_addon_pairs.js (left as it is) plus the device-grouping entry points of
 * csrc/ht_napi.cc — detectBestEnqueue, collectBestDevice, detectGrouped, detectBestRecords — on the CPU oracle, so that the host logic of
 * new ccv.DeviceBatch(.., {grouping: 'device'}) runs without a GPU.  The call-sequence rules are those of ht_detect_best_*: status -6
 * (HT_ERR_STATE) in the message when no batch is in flight, when no grouping was enqueued behind it, or when the grouped lists asked for
 * belong to a batch whose buffers a later grouping has taken over (the requeue form).  The grouped list of a frame is the facade's own port
 * of ccv's grouping (ccv._group, itself checked against the reference's recorded vectors by tests/js/parity_cpu.js) on the oracle's raw hits;
 * the best face is the oracle's.  groupHits is not mocked: DeviceBatch does not use it.  `withGroup(false)` is an addon that lacks the calls. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_pairs.js'));
const oracle = require(path.join(__dirname, 'oracle_addon.node'));
const root = path.join(__dirname, '..', '..');

function count(name) { mock.calls[name] = (mock.calls[name] || 0) + 1; }
function live(c) { if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context'); return c; }
function i32(v, what) { if (typeof v !== 'number' || v !== (v | 0)) throw new TypeError('mock addon: ' + what); return v; }

const groupFns = {
  detectBestEnqueue: function (c, minNeighbors, frameBase) {
    count('detectBestEnqueue'); live(c);
    i32(minNeighbors, 'detectBestEnqueue(ctx, minNeighbors, frameBase = 0)');
    if (!c.enqueued) throw new Error('mock addon: status -6: no detect batch in flight');
    c.enqueued.best = { mn: minNeighbors, base: frameBase === undefined ? 0 : i32(frameBase, 'frameBase') };
  },
  collectBestDevice: function (c, requeueFlags) {
    count('collectBestDevice'); live(c);
    if (!c.enqueued) throw new Error('mock addon: status -6: nothing enqueued');
    if (!c.enqueued.best) throw new Error('mock addon: status -6: no detectBestEnqueue behind the batch in flight');
    const e = c.enqueued, g = e.best;
    const r = mock.collectBest(c, g.mn, -1); /* the oracle's best faces; bookkeeping (whitebalance snapshot) as for every collect */
    mock.calls.collectBest--;                /* ... but not a call the host made */
    c.grouped = { frames: e.frames, n: e.n, stride: e.stride, flags: e.flags, mn: g.mn, base: g.base, best: r.best };
    if (requeueFlags !== undefined && requeueFlags >= 0) {
      if (!c.frames || c.n < 1) throw new Error('mock addon: no frames bound');
      c.enqueued = { flags: requeueFlags, frames: c.frames, n: c.n, stride: c.stride, best: { mn: g.mn, base: g.base } };
      c.grouped.lists = false; /* the next grouping has taken the device buffers over */
    }
    return r;
  },
  detectGrouped: function (c, frame) {
    count('detectGrouped'); live(c);
    i32(frame, 'detectGrouped(ctx, frame)');
    const G = c.grouped;
    if (!G || G.lists === false) throw new Error('mock addon: status -6: no device-grouped batch');
    if (frame < 0 || frame >= G.n) throw new Error('mock addon: status -1: frame outside the collected batch');
    const ccv = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js')).ccv;
    const h = oracle.detectRaw(G.frames.subarray(frame * G.stride, frame * G.stride + c.w * c.h * 4), c.w, c.h, G.flags & 1, c.cascade, c.interval);
    const list = ccv._group(ccv._hitsToSeq(h, 0, h.sum.length, { width: 24, height: 24 }, c.interval), G.mn), out = new Float64Array(6 * list.length);
    list.forEach(function (r, k) { out.set([r.x, r.y, r.width, r.height, r.confidence, G.mn > 0 ? r.neighbors : 1], 6 * k); });
    return out;
  },
  detectBestRecords: function (c) {
    count('detectBestRecords'); live(c);
    const G = c.grouped;
    if (!G) throw new Error('mock addon: status -6: no device-grouped batch');
    const out = new Float64Array(8 * G.n);
    for (let f = 0; f < G.n; f++) { out.set(G.best.subarray(6 * f, 6 * f + 6), 8 * f); out[8 * f + 6] = G.base + f; out[8 * f + 7] = 1; }
    return out;
  }
};

mock.withGroup = function (on) {
  Object.keys(groupFns).forEach(function (k) { if (on) mock[k] = groupFns[k]; else delete mock[k]; });
  return mock;
};
mock.withGroup(true);
module.exports = mock;
