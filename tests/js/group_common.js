'use strict';
/* tests/js/group_common.js — the comparisons tests/js/group_cpu.js (oracle-backed mock addon) and tests/js/group_gpu.js (product addon,
 * MI355X) share: a ccv.DeviceBatch with {grouping: 'device'} next to one with the default host route on the same frames — detectBest,
 * detect, whitebalance, the step functions of the C5 loop — and both against what the job file expects (best faces from the CPU oracle,
 * grouped lists as the reference recorded them).  job: {w, h, n, frames: file of n*w*h*4 bytes, expect_best: [6 n], expect_grouped:
 * [[{x, y, width, height, confidence, neighbors}, ...] per frame] for min_neighbors 1}. */
const fs = require('fs');

module.exports = function (headtrackr, job, out, check) {
  const frames = new Uint8Array(fs.readFileSync(job.frames));
  const make = function (grouping, depth) {
    const o = { depth: depth };
    if (grouping) o.grouping = grouping;
    const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, o);
    b.upload(frames, 0);
    return b;
  };
  const plain = function (v) { /* typed arrays and nested results as plain JSON: equal text <=> equal doubles */
    if (ArrayBuffer.isView(v)) return Array.from(v);
    if (Array.isArray(v)) return v.map(plain);
    if (v && typeof v === 'object') { const o = {}; Object.keys(v).sort().forEach(function (k) { o[k] = plain(v[k]); }); return o; }
    return v;
  };
  const same = function (what, a, b) { out.compared++; return check(JSON.stringify(plain(a)) === JSON.stringify(plain(b)), what + ': device route differs from host route'); };

  const host = make(undefined, 2), dev = make('device', 2);
  check(host.grouping === 'host' && dev.grouping === 'device', 'DeviceBatch.grouping');

  /* detectBest: several batches over two contexts (enqueue, requeue inside the collect call, final collect) */
  [[5, 1], [1, 2], [3, 0]].forEach(function (bm) {
    const a = host.detectBest(bm[0], bm[1], 0), b = dev.detectBest(bm[0], bm[1], 0);
    same('detectBest(' + bm + ').best', a.best, b.best);
    same('detectBest(' + bm + ').hits', a.hits, b.hits);
    check(b.batches === bm[0] && b.best.length === 6 * job.n, 'detectBest result shape');
    if (bm[1] === 1) { out.compared++; check(JSON.stringify(plain(b.best)) === JSON.stringify(job.expect_best), 'detectBest: device route differs from the oracle'); }
  });

  /* detect: the full grouped lists */
  [1, 0, 2].forEach(function (mn) {
    const a = host.detect(mn, 0), b = dev.detect(mn, 0);
    same('detect(' + mn + ')', a, b);
    if (mn === 1) {
      out.compared++;
      const got = b.map(function (list) { return list.map(function (r) { return [r.x, r.y, r.width, r.height, r.confidence, r.neighbors]; }); });
      const want = job.expect_grouped.map(function (list) { return list.map(function (r) { return [r.x, r.y, r.width, r.height, r.confidence, r.neighbors]; }); });
      check(JSON.stringify(got) === JSON.stringify(want), 'detect(1): device route differs from the recorded grouped rects');
      out.grouped_rects = got.reduce(function (s, l) { return s + l.length; }, 0);
    }
  });

  same('whitebalance', host.whitebalance(0), dev.whitebalance(0));
  host.destroy(); dev.destroy();

  /* the C5 loop's step functions on one context */
  const h1 = make(undefined, 1), d1 = make('device', 1);
  let a = h1.detectStep(0, 1), b = d1.detectStep(0, 1);
  same('detectStep.best', a.best, b.best); same('detectStep.rects', a.rects, b.rects); same('detectStep.hits', a.hits, b.hits);
  same('trackStep', h1.trackStep(0, true), d1.trackStep(0, true));
  h1.detectStepEnqueue(0); d1.detectStepEnqueue(0); /* grouping enqueued with the default min_neighbors; finish asks for another */
  a = h1.detectStepFinish(2); b = d1.detectStepFinish(2);
  same('detectStepEnqueue + detectStepFinish(2).best', a.best, b.best); same('detectStepFinish(2).rects', a.rects, b.rects);
  h1.trackEnqueue(0, true); d1.trackEnqueue(0, true);
  h1.detectStepEnqueue(0, 1); d1.detectStepEnqueue(0, 1); /* the detect of the next step behind a track step in flight */
  same('trackCollect', h1.trackCollect(), d1.trackCollect());
  a = h1.detectStepFinish(1, { feeds: job.feeds }); b = d1.detectStepFinish(1, { feeds: job.feeds });
  same('detectStepFinish({feeds}).best', a.best, b.best); same('.initialised', a.initialised, b.initialised); same('.rects', a.rects, b.rects);
  out.initialised = b.initialised.length;
  h1.destroy(); d1.destroy();
};
