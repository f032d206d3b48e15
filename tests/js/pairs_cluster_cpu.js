'use strict';
/* The cluster pair schedule's JavaScript layer on the oracle-backed mock addon (driven by tests/test_cs_pairs_cluster_cpu.py; no GPU):
 *     node tests/js/pairs_cluster_cpu.js job.json
 * tests/js/pairs_cluster_common.js: which options reach createContext, the refused values, and the existing pairs job — on the mock the
 * option changes nothing, so the MultiTracker and DeviceBatch runs must return what they return today.  Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_pairs.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], calls_exact: 0, calls_total: 0, loop_detects: 0, loop_lost: 0, multi_done: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }

require(path.join(__dirname, 'pairs_cluster_common.js'))(mock, headtrackr, Canvas, job, out, check);
out.pair_calls = [mock.calls.camshiftInitPairs || 0, mock.calls.camshiftTrackPairs || 0];
process.stdout.write(JSON.stringify(out) + '\n');
