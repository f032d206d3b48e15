'use strict';
/* CPU-side checks of the JavaScript layer of the per-face initTracker (driven by tests/test_init_faces_cpu.py; no GPU):
 *     node tests/js/init_faces_cpu.js job.json
 *  1. tests/js/init_faces_common.js on the oracle-backed mock addon (tests/js/mock_addon_init_faces.js): DeviceBatch.initFaces /
 *     initFacesResult against the Python restatement's records — the expectations of the GPU run (tests/js/init_faces_gpu.js);
 *  2. a frame that is not final while its batch is in flight: its slots are deferred, stay deferred while the batch is in flight, and
 *     are retried by initFacesResult once detectStepFinish has collected it — the other frames' slots are not initialised twice — and a
 *     further read returns the same records of the whole pair list without another call to the addon;
 *  3. the refusals: grouping 'host', an addon without the calls, a NaN threshold, initFacesResult without a call — none reaches the addon.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_init_faces.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], compared: 0, deferred: 0, retried: 0, reread: 0, refusals: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }

try {
  require(path.join(__dirname, 'init_faces_common.js'))(headtrackr, job, out, check);

  { /* 2. deferred, then retried */
    const call = job.calls[0], pairs = Int32Array.from(call.pairs), np = pairs.length >> 1, f0 = job.deferFrame;
    const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, grouping: 'device', trackers: job.trackers });
    b.upload(new Uint8Array(fs.readFileSync(job.frames)), 0);
    mock.csfDeferFrames = [f0];
    b.detectStepEnqueue(0, 1);
    b.initFaces(pairs, { minConfidence: call.minConfidence, associate: call.associate });
    const early = b.initFacesResult(), calls0 = mock.calls.camshiftInitFaces;
    for (let i = 0; i < np; i++) {
      const deferred = pairs[2 * i + 1] === f0;
      if (deferred) { out.deferred++; check(early[8 * i] === mock.CSB_DEFERRED && early[8 * i + 1] === -1 && early[8 * i + 6] === 0, 'pair ' + i + ' must be deferred'); }
      else for (let k = 0; k < 8; k++) check(early[8 * i + k] === call.expect[8 * i + k], 'pair ' + i + ' of a final frame, word ' + k);
    }
    check(mock.calls.camshiftInitFaces === calls0, 'initFacesResult retried while the batch was in flight');
    b.detectStepFinish(1);
    const late = b.initFacesResult();
    check(mock.calls.camshiftInitFaces === calls0 + 1, 'exactly one retry after the collect');
    const retried = mock.calls.camshiftInitFaces === calls0 + 1;
    for (let i = 0; i < 8 * np; i++) if (!check(late[i] === call.expect[i], 'after the retry: record word ' + i + ' is ' + late[i] + ', expected ' + call.expect[i])) break;
    const again = b.initFacesResult(); /* repeatable after the retry: the whole pair list again, and nothing more reaches the device */
    check(again instanceof Int32Array && again.length === 8 * np, 'second read after the retry: ' + again.length + ' words, expected ' + 8 * np);
    for (let i = 0; i < 8 * np; i++) if (!check(again[i] === call.expect[i], 'second read after the retry: record word ' + i)) break;
    check(again !== late, 'the reads share one array');
    check(mock.calls.camshiftInitFaces === calls0 + 1, 'a second read after the retry called camshiftInitFaces again');
    if (again.length === 8 * np && mock.calls.camshiftInitFaces === calls0 + 1) out.reread = 1;
    if (retried) out.retried = out.deferred;
    mock.csfDeferFrames = [];
    b.destroy();
  }

  { /* 3. refusals */
    const pairs = Int32Array.from(job.calls[0].pairs);
    const refused = function (what, type, re, fn) {
      const before = JSON.stringify(mock.calls);
      let ok = false;
      try { fn(); } catch (e) { ok = e instanceof type && re.test(e.message); }
      if (check(ok, what + ' must throw a ' + type.name + ' matching ' + re) && check(JSON.stringify(mock.calls) === before, what + ' reached the addon')) out.refusals++;
    };
    const h = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, trackers: job.trackers }); /* grouping: 'host' */
    refused("initFaces under grouping 'host'", RangeError, /grouping: 'device'/, function () { h.initFaces(pairs); });
    refused("initFacesResult under grouping 'host'", RangeError, /grouping: 'device'/, function () { h.initFacesResult(); });
    h.destroy();
    const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, grouping: 'device', trackers: job.trackers });
    refused('initFacesResult without a call', Error, /no initFaces/, function () { b.initFacesResult(); });
    refused('a NaN threshold', RangeError, /NaN/, function () { b.initFaces(pairs, { minConfidence: NaN }); });
    refused('pairs that are no Int32Array', TypeError, /Int32Array/, function () { b.initFaces([8, 0]); });
    mock.withInitFaces(false);
    refused('an addon without the calls', Error, /camshiftInitFaces/, function () { b.initFaces(pairs); });
    mock.withInitFaces(true);
    b.destroy();
  }
} catch (e) {
  check(false, 'exception: ' + (e && e.stack ? e.stack : e));
}
console.log(JSON.stringify(out));
