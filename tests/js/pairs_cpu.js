'use strict';
/* CPU-side checks of the JavaScript layer of the (stream, frame) pair calls (driven by tests/test_pairs_cpu.py; no GPU):
 *     node tests/js/pairs_cpu.js job.json
 *  1. tests/js/pairs_common.js on the oracle-backed mock addon (tests/js/mock_addon_pairs.js): ccv.DeviceBatch initPairs / trackPairs /
 *     trackPairsEnqueue + trackCollect, detectStepFinish(.., {feeds}) in the per-feed-state loop, camshift.MultiTracker — the expectations
 *     of the GPU run (tests/js/pairs_gpu.js);
 *  2. a DeviceBatch used WITHOUT the new options makes exactly the addon calls it made before;
 *  3. on an addon without the pair calls (withPairs(false)) the new methods throw an Error that names what is missing, before anything
 *     reaches the addon.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_pairs.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], calls_exact: 0, calls_total: 0, loop_detects: 0, loop_lost: 0, multi_done: 0, legacy_calls: null, missing_checks: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }

require(path.join(__dirname, 'pairs_common.js'))(headtrackr, Canvas, job, out, check);
out.pair_calls = [mock.calls.camshiftInitPairs || 0, mock.calls.camshiftTrackPairs || 0];

/* 2. the old surface, old calls */
{
  const J = job.loop, before = Object.assign({}, mock.calls), delta = {};
  const b = new headtrackr.ccv.DeviceBatch(J.w, J.h, J.n, { depth: 1 });
  b.upload(new Uint8Array(fs.readFileSync(J.sets[0])), 0);
  const r = b.detectStep(0);
  check(r.rects.length === 4 * J.n && r.initialised === undefined, 'detectStep without {feeds}: rects for every feed');
  check(b.trackStep(0, true).length === 9 * J.n, 'trackStep');
  b.trackEnqueue(0, true);
  check(b.trackCollect().length === 9 * J.n, 'trackEnqueue + trackCollect');
  b.destroy();
  Object.keys(mock.calls).forEach(function (k) { if (mock.calls[k] !== (before[k] || 0)) delta[k] = mock.calls[k] - (before[k] || 0); });
  out.legacy_calls = delta;
}

/* 3. an addon without the pair calls */
{
  mock.withPairs(false);
  const J = job.loop, before = JSON.stringify(mock.calls);
  const b = new headtrackr.ccv.DeviceBatch(J.w, J.h, J.n, { depth: 1 });
  const created = JSON.stringify(mock.calls);
  ['initPairs', 'trackPairs', 'trackPairsEnqueue'].forEach(function (m) {
    let threw = false;
    try { b[m](0, new Int32Array([0, 0]), new Int32Array([1, 1, 4, 4])); } catch (e) { threw = /camshiftInitPairs/.test(e.message); }
    if (check(threw, m + ' on an addon without the pair calls must throw')) out.missing_checks++;
  });
  check(JSON.stringify(mock.calls) === created && created !== before, 'the refused calls did not reach the addon');
  b.destroy();
  let threw = false;
  try { new headtrackr.camshift.MultiTracker().initTracker(new Canvas(8, 8), [new headtrackr.camshift.Rectangle(1, 1, 4, 4)]); } catch (e) { threw = /camshiftInitPairs/.test(e.message); }
  if (check(threw, 'MultiTracker.initTracker on an addon without the pair calls must throw')) out.missing_checks++;
  mock.withPairs(true);
}

process.stdout.write(JSON.stringify(out) + '\n');
