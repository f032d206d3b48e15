'use strict';
/* The JavaScript side of the (stream, frame) pair tests, shared by tests/js/pairs_cpu.js (oracle-backed mock addon) and
 * tests/js/pairs_gpu.js (product addon on a GPU): the same calls against the same expectations, which come from the CPU oracle through
 * the job file (tests/test_pairs_cpu.py / tests/test_gpu_camshift_pairs.py write it).
 * job: { angle_tol,
 *        batch: {w, h, n, trackers, sets[raw files of n frames], init_pairs[], rects[], calls[{set, pairs[], expect[{to[5], sw[4]}]}]},
 *        loop:  {w, h, n, sets[raw file per step], expect[feed][step] = {mode 'VJ', best[5], found} | {mode 'CS', to[5], sw[4], lost}},
 *        multi: [{name, w, h, rects[[4]], frames[raw files], trackers[[{x, y, width, height, angle, sw[4]}]]}] }
 * Every integer-valued output must be EQUAL; the angle may differ by angle_tol (modulo pi) and is not compared on a lost call (0 x 0). */
const fs = require('fs');

module.exports = function run(headtrackr, Canvas, job, out, check) {
  const tol = job.angle_tol;
  function sameCall(r, o, want, what) { /* r[o .. o+9) against {to, sw, lost} */
    let ok = true;
    for (let k = 0; k < 4; k++) ok = check(r[o + k] === want.to[k], what + ': track object [' + k + '] ' + r[o + k] + ' != ' + want.to[k]) && ok;
    for (let k = 0; k < 4; k++) ok = check(r[o + 5 + k] === want.sw[k], what + ': search window [' + k + '] ' + r[o + 5 + k] + ' != ' + want.sw[k]) && ok;
    if (!want.lost) {
      let d = Math.abs(r[o + 4] - want.to[4]);
      d = Math.min(d, Math.abs(d - Math.PI));
      ok = check(d <= tol, what + ': angle ' + r[o + 4] + ' vs ' + want.to[4]) && ok;
    }
    if (ok) out.calls_exact++;
    out.calls_total++;
    return ok;
  }

  /* ---- ccv.DeviceBatch: initPairs / trackPairs / trackPairsEnqueue + trackCollect ---- */
  {
    const J = job.batch;
    const b = new headtrackr.ccv.DeviceBatch(J.w, J.h, J.n, { depth: 1, sets: J.sets.length, trackers: J.trackers });
    J.sets.forEach(function (f, k) { b.upload(new Uint8Array(fs.readFileSync(f)), k); });
    b.initPairs(0, new Int32Array(J.init_pairs), new Int32Array(J.rects));
    const half = J.calls.length >> 1;
    J.calls.slice(0, half).forEach(function (c, k) {
      const r = b.trackPairs(c.set, new Int32Array(c.pairs), true);
      check(r instanceof Float64Array && r.length === 9 * c.expect.length, 'trackPairs: Float64Array(9 n)');
      c.expect.forEach(function (w, i) { sameCall(r, 9 * i, w, 'batch call ' + k + ' pair ' + i); });
    });
    /* the remaining calls are all enqueued before the first is collected: the search windows that link them live on the device */
    J.calls.slice(half).forEach(function (c) { check(b.trackPairsEnqueue(c.set, new Int32Array(c.pairs), true) === undefined, 'trackPairsEnqueue returns nothing'); });
    J.calls.slice(half).forEach(function (c, k) {
      const r = b.trackCollect();
      check(r.length === 9 * c.expect.length, 'trackCollect of a pair step: 9 x pairs');
      c.expect.forEach(function (w, i) { sameCall(r, 9 * i, w, 'batch enqueued call ' + (half + k) + ' pair ' + i); });
    });
    let threw = false;
    try { b.trackPairs(0, new Int32Array([0, 0, 0, 1]), true); } catch (e) { threw = /status -1/.test(e.message); }
    check(threw, 'a duplicate stream is refused with status -1');
    threw = false;
    try { b.trackPairs(0, [0, 0], true); } catch (e) { threw = e instanceof TypeError; }
    check(threw, 'pairs that are no Int32Array are a TypeError');
    b.destroy();
    out.batch_done = true;
  }

  /* ---- the per-feed-state loop through DeviceBatch: detectStepFinish(.., {feeds}) + trackPairs ---- */
  {
    const J = job.loop, n = J.n;
    const b = new headtrackr.ccv.DeviceBatch(J.w, J.h, n, { depth: 1, sets: J.sets.length });
    J.sets.forEach(function (f, k) { b.upload(new Uint8Array(fs.readFileSync(f)), k); });
    const tracking = [];
    for (let f = 0; f < n; f++) tracking.push(false);
    out.loop_mixed_steps = 0;
    for (let k = 0; k < J.sets.length; k++) {
      const D = [], T = [];
      for (let f = 0; f < n; f++) (tracking[f] ? T : D).push(f);
      if (D.length && T.length) out.loop_mixed_steps++;
      D.forEach(function (f) { check(J.expect[f][k].mode === 'VJ', 'step ' + k + ' feed ' + f + ': the host detects, the oracle loop tracks'); });
      T.forEach(function (f) { check(J.expect[f][k].mode === 'CS', 'step ' + k + ' feed ' + f + ': the host tracks, the oracle loop detects'); });
      if (D.length) {
        b.detectStepEnqueue(k);
        const r = b.detectStepFinish(1, { feeds: D });
        check(r.best.length === 6 * n, 'detectStepFinish returns best for all feeds');
        const found = [];
        D.forEach(function (f) {
          const e = J.expect[f][k];
          for (let q = 0; q < 5; q++) check(r.best[6 * f + q] === e.best[q], 'step ' + k + ' feed ' + f + ': best[' + q + '] ' + r.best[6 * f + q] + ' != ' + e.best[q]);
          if (e.found) found.push(f);
        });
        check(JSON.stringify(r.initialised) === JSON.stringify(found), 'step ' + k + ': initialised ' + JSON.stringify(r.initialised) + ' != ' + JSON.stringify(found));
        found.forEach(function (f) { tracking[f] = true; });
        out.loop_detects += D.length;
      }
      if (T.length) {
        const pr = new Int32Array(2 * T.length);
        T.forEach(function (f, i) { pr[2 * i] = f; pr[2 * i + 1] = f; });
        const r = b.trackPairs(k, pr, true);
        T.forEach(function (f, i) {
          const e = J.expect[f][k];
          if (e.mode !== 'CS') return;
          sameCall(r, 9 * i, e, 'loop step ' + k + ' feed ' + f);
          const lost = r[9 * i + 2] === 0 || r[9 * i + 3] === 0; /* main.js:229 */
          check(lost === e.lost, 'loop step ' + k + ' feed ' + f + ': lost ' + lost + ' != ' + e.lost);
          if (lost) { tracking[f] = false; out.loop_lost++; }
        });
      }
    }
    b.destroy();
  }

  /* ---- camshift.MultiTracker against the recording of M reference camshift.Tracker instances on one canvas ---- */
  job.multi.forEach(function (g) {
    const canvasOf = function (file) { return new Canvas(g.w, g.h).setFrame(fs.readFileSync(file)); };
    const mt = new headtrackr.camshift.MultiTracker({ calcAngles: true });
    mt.initTracker(canvasOf(g.frames[0]), g.rects.map(function (r) { return new headtrackr.camshift.Rectangle(r[0], r[1], r[2], r[3]); }));
    check(mt.count() === g.rects.length, g.name + ': one tracker per rect');
    g.rects.forEach(function (r, j) { /* camshift.js:209-210 */
      const sw = mt.getSearchWindow(j), o = mt.getTrackObj(j);
      check(sw.x === r[0] && sw.y === r[1] && sw.width === r[2] && sw.height === r[3] && o.width === 0 && o.height === 0 && o.x === 0 && o.y === 0,
        g.name + ': state after initTracker');
    });
    for (let k = 1; k < g.frames.length; k++) {
      mt.track(canvasOf(g.frames[k]));
      g.trackers.forEach(function (calls, j) {
        const w = calls[k - 1], o = mt.getTrackObj(j), sw = mt.getSearchWindow(j);
        sameCall([o.x, o.y, o.width, o.height, o.angle, sw.x, sw.y, sw.width, sw.height], 0, { to: [w.x, w.y, w.width, w.height, w.angle], sw: w.sw, lost: false },
          g.name + ' tracker ' + j + ' call ' + k);
      });
    }
    mt.release();
    out.multi_done++;
  });
};
