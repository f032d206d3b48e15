'use strict';
/* tests/js/init_best_common.js — the comparisons tests/js/init_best_cpu.js (oracle-backed mock addon) and tests/js/init_best_gpu.js
 * (product addon, MI355X) share: a ccv.DeviceBatch with {grouping: 'device', handoff: 'device'} next to the default one on the same
 * frames.  Under handoff 'device' the trackers change at the ENQUEUE point in stream order, so a sequence enqueue -> track -> finish is
 * compared with the default route's drained sequence enqueue -> finish -> track.  Every result must be JSON-equal.
 * job: tests/group_cases.py js_job: {w, h, n, frames: file of n*w*h*4 bytes, feeds}. */
const fs = require('fs');

module.exports = function (headtrackr, job, out, check) {
  const frames = new Uint8Array(fs.readFileSync(job.frames)), fb = job.w * job.h * 4;
  const plain = function (v) {
    if (ArrayBuffer.isView(v)) return Array.from(v);
    if (Array.isArray(v)) return v.map(plain);
    if (v && typeof v === 'object') { const o = {}; Object.keys(v).sort().forEach(function (k) { o[k] = plain(v[k]); }); return o; }
    return v;
  };
  const same = function (what, a, b) { out.compared++; return check(JSON.stringify(plain(a)) === JSON.stringify(plain(b)), what + ': device hand-off differs from the host hand-off'); };
  const make = function (device) {
    const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, device ? { depth: 1, grouping: 'device', handoff: 'device' } : { depth: 1 });
    b.upload(frames, 0);
    return b;
  };
  const host = make(false), dev = make(true);
  check(host.handoff === 'host' && dev.handoff === 'device' && dev.grouping === 'device', 'DeviceBatch.handoff');

  /* detectStep = enqueue + finish: every feed, centre-half fallback for the feed without a face */
  let a = host.detectStep(0, 1), b = dev.detectStep(0, 1);
  same('detectStep', a, b);
  out.fallbacks = 0;
  for (let f = 0; f < job.n; f++) if (!(b.best[6 * f + 5] > 0)) { out.fallbacks++; check(b.rects[4 * f] === job.w >> 2 && b.rects[4 * f + 3] === job.h >> 1, 'centre-half fallback of feed ' + f); }
  same('trackStep', host.trackStep(0, true), dev.trackStep(0, true));

  /* enqueue -> track -> finish -> collect against the drained host sequence, without and with {feeds} */
  [undefined, { feeds: job.feeds }, { feeds: [] }].forEach(function (sel) {
    const tag = sel ? 'feeds [' + sel.feeds + ']' : 'every feed';
    host.detectStepEnqueue(0, 1);
    a = host.detectStepFinish(1, sel);
    host.trackEnqueue(0, true);
    const ta = host.trackCollect();
    dev.detectStepEnqueue(0, 1, sel);
    dev.trackEnqueue(0, true); /* at once: the best faces have not crossed to the host */
    b = dev.detectStepFinish(1, sel);
    const tb = dev.trackCollect();
    same('detectStepFinish, ' + tag, a, b);
    same('track step behind the enqueue, ' + tag, ta, tb);
    if (sel && sel.feeds.length) out.initialised = b.initialised.length;
  });

  /* a finish that does not match its enqueue: the trackers are already initialised */
  const rangeError = function (what, fn) { let ok = false; try { fn(); } catch (e) { ok = e instanceof RangeError; } if (check(ok, what + ' must be a RangeError')) out.range_errors++; };
  dev.detectStepEnqueue(0, 1);
  rangeError('detectStepFinish with another min_neighbors', function () { dev.detectStepFinish(2); });
  rangeError('detectStepFinish with a sel the enqueue did not have', function () { dev.detectStepFinish(1, { feeds: job.feeds }); });
  same('... and the matching finish still works', host.detectStep(0, 1), dev.detectStepFinish(1));
  dev.detectStepEnqueue(0, 1, { feeds: job.feeds });
  rangeError('detectStepFinish without the sel of the enqueue', function () { dev.detectStepFinish(1); });
  rangeError('detectStepFinish with other feeds', function () { dev.detectStepFinish(1, { feeds: job.feeds.slice(1) }); });
  dev.detectStepFinish(1, { feeds: job.feeds });
  rangeError('a feed outside the batch', function () { dev.detectStepEnqueue(0, 1, { feeds: [job.n] }); });
  rangeError("handoff: 'gpu'", function () { new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { grouping: 'device', handoff: 'gpu' }); });
  rangeError("handoff: 'device' without grouping: 'device'", function () { new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { handoff: 'device' }); });
  host.destroy(); dev.destroy();

  /* a mini C5 loop: two feeds, 35 steps over two frame sets, a detect step every 30th, two track steps outstanding.  The host arm drains
   * its queue in front of every detect step, as benchlib/c5.py does; the device arm enqueues detect, grouping and initTracker behind the
   * outstanding track steps and collects the best faces one step later. */
  const loop = function (device) {
    const o = device ? { depth: 1, sets: 2, grouping: 'device', handoff: 'device' } : { depth: 1, sets: 2 };
    const B = new headtrackr.ccv.DeviceBatch(job.w, job.h, 2, o);
    B.upload(frames.subarray(0, 2 * fb), 0); B.upload(frames.subarray(2 * fb, 4 * fb), 1);
    const res = { detects: [], tracks: [] };
    let pending = 0, unfinished = false;
    for (let i = 0; i < 35; i++) {
      const set = i & 1;
      if (i % 30 === 0) {
        if (device) { B.detectStepEnqueue(set, 1); unfinished = true; continue; }
        while (pending) { res.tracks.push(B.trackCollect()); pending--; }
        res.detects.push(B.detectStep(set, 1));
        continue;
      }
      B.trackEnqueue(set, true); pending++;
      if (unfinished) { res.detects.push(B.detectStepFinish(1)); unfinished = false; }
      while (pending > 2) { res.tracks.push(B.trackCollect()); pending--; }
    }
    while (pending) { res.tracks.push(B.trackCollect()); pending--; }
    B.destroy();
    return res;
  };
  const la = loop(false), lb = loop(true);
  check(la.detects.length === 2 && la.tracks.length === 33, 'mini C5 loop: 2 detect steps and 33 track steps');
  same('mini C5 loop: detect steps', la.detects, lb.detects);
  same('mini C5 loop: track steps', la.tracks, lb.tracks);
  out.loop_tracks = lb.tracks.length;
};
