'use strict';
/* The (stream, frame) pair calls from the JavaScript host, on a GPU (driven by tests/test_gpu_camshift_pairs.py):
 *     node tests/js/pairs_gpu.js job.json
 * tests/js/pairs_common.js on the product addon: ccv.DeviceBatch initPairs / trackPairs / trackPairsEnqueue + trackCollect, the
 * per-feed-state loop through detectStepFinish(.., {feeds}), and camshift.MultiTracker against tests/golden/multitrack.json — the same
 * expectations as tests/js/pairs_cpu.js on the mock.  The addon's pair functions are wrapped here to count that the facade really went
 * through them.  Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], calls_exact: 0, calls_total: 0, loop_detects: 0, loop_lost: 0, multi_done: 0, pair_calls: [0, 0] };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }

const realInit = A.camshiftInitPairs, realTrack = A.camshiftTrackPairs;
if (check(typeof realInit === 'function' && typeof realTrack === 'function', 'addon exports camshiftInitPairs / camshiftTrackPairs')) {
  A.camshiftInitPairs = function () { out.pair_calls[0]++; return realInit.apply(this, arguments); };
  A.camshiftTrackPairs = function () { out.pair_calls[1]++; return realTrack.apply(this, arguments); };
  try {
    require(path.join(__dirname, 'pairs_common.js'))(headtrackr, Canvas, job, out, check);
  } catch (e) { check(false, 'exception: ' + (e && e.stack ? e.stack : e)); }
}

process.stdout.write(JSON.stringify(out) + '\n', function () { headtrackr.exitNow(out.ok ? 0 : 1); });
