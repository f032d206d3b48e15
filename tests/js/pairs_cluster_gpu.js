'use strict';
/* The cluster pair schedule from the JavaScript host, on a GPU (driven by tests/test_gpu_cs_pairs_cluster.py):
 *     node tests/js/pairs_cluster_gpu.js job.json
 * tests/js/pairs_cluster_common.js on the product addon: the existing pairs job (batch part, per-feed-state loop, camshift.MultiTracker)
 * with {pairSchedule: 'cluster'} / headtrackr.camshift.pairSchedule = 'cluster'.  The addon's pair functions are wrapped to count that
 * the facade went through them.  Prints one JSON line. */
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
A.camshiftInitPairs = function () { out.pair_calls[0]++; return realInit.apply(this, arguments); };
A.camshiftTrackPairs = function () { out.pair_calls[1]++; return realTrack.apply(this, arguments); };
try {
  require(path.join(__dirname, 'pairs_cluster_common.js'))(A, headtrackr, Canvas, job, out, check);
} catch (e) { check(false, 'exception: ' + (e && e.stack ? e.stack : e)); }

process.stdout.write(JSON.stringify(out) + '\n', function () { headtrackr.exitNow(out.ok ? 0 : 1); });
