'use strict';
/* The DeviceBatch route of the per-face initTracker against the expectations tests/init_faces_cases.py computed (the rule restated in
 * Python on the CPU oracle's grouped lists), on whatever addon `headtrackr` found: tests/js/init_faces_cpu.js (mock) and
 * tests/js/init_faces_gpu.js (product addon) both run this.  job.calls: [{pairs, minConfidence, associate, expect: 8 int32 per pair}], one
 * detect step and one initFaces each, in order on ONE DeviceBatch — a call's association sees the trackers the calls before it left. */
const fs = require('fs');
module.exports = function (headtrackr, job, out, check) {
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, grouping: 'device', trackers: job.trackers });
  b.upload(new Uint8Array(fs.readFileSync(job.frames)), 0);
  job.calls.forEach(function (call, ci) {
    const pairs = Int32Array.from(call.pairs), np = pairs.length >> 1;
    b.detectStepEnqueue(0, 1);
    b.initFaces(pairs, { minConfidence: call.minConfidence, associate: call.associate });
    const early = b.initFacesResult();               /* while the batch is in flight */
    b.trackPairsEnqueue(0, Int32Array.from(call.track), true); /* a track step right behind it: nothing waited for */
    b.detectStepFinish(1);
    const t = b.trackCollect();
    const late = b.initFacesResult();                /* repeatable, and the same after the collect */
    check(early instanceof Int32Array && early.length === 8 * np, 'call ' + ci + ': result shape');
    for (let i = 0; i < 8 * np; i++) {
      if (!check(early[i] === call.expect[i], 'call ' + ci + ': record word ' + i + ' is ' + early[i] + ', expected ' + call.expect[i])) break;
      if (!check(late[i] === early[i], 'call ' + ci + ': the result changed between two reads')) break;
    }
    for (let i = 0; i < (call.track.length >> 1); i++) { /* the tracked slots sit on the faces they were given */
      const k = call.pairs.indexOf(call.track[2 * i]) >> 1, w = [t[9 * i + 5], t[9 * i + 6], t[9 * i + 7], t[9 * i + 8]];
      const r = call.expect.slice(8 * k + 2, 8 * k + 6);
      const ow = Math.min(w[0] + w[2], r[0] + r[2]) - Math.max(w[0], r[0]), oh = Math.min(w[1] + w[3], r[1] + r[3]) - Math.max(w[1], r[1]);
      check(ow > 0 && oh > 0, 'call ' + ci + ': tracked slot ' + k + ' left its face: window ' + w + ', rect ' + r);
    }
    out.compared += np;
  });
  b.destroy();
};
