'use strict';
/* CPU-side checks of the JavaScript layer of the device hand-off (driven by tests/test_init_best_cpu.py; no GPU):
 *     node tests/js/init_best_cpu.js job.json
 *  1. tests/js/init_best_common.js on the oracle-backed mock addon (tests/js/mock_addon_init_best.js): {grouping: 'device', handoff:
 *     'device'} returns what the default returns — the expectations of the GPU run (tests/js/init_best_gpu.js);
 *  2. under handoff 'device' the mock sees no camshiftInitPairs and no camshiftInitBound, the default none of the new calls;
 *  3. on an addon without the new calls (withInitBest(false)) handoff 'device' throws an Error that names what is missing before anything
 *     reaches the addon, and the default still works.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_init_best.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], compared: 0, range_errors: 0, host_calls: null, device_calls: null, missing_checks: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const NEW = ['camshiftInitBest', 'camshiftInitBestResult'];

require(path.join(__dirname, 'init_best_common.js'))(headtrackr, job, out, check);

function callsOf(device) {
  const before = Object.assign({}, mock.calls), delta = {};
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, device ? { depth: 1, grouping: 'device', handoff: 'device' } : { depth: 1 });
  b.upload(new Uint8Array(fs.readFileSync(job.frames)), 0);
  b.detectStep(0, 1); b.trackStep(0, true);
  b.detectStepEnqueue(0, 1, { feeds: job.feeds }); b.trackEnqueue(0, true); b.detectStepFinish(1, { feeds: job.feeds }); b.trackCollect();
  b.destroy();
  Object.keys(mock.calls).forEach(function (k) { if (mock.calls[k] !== (before[k] || 0)) delta[k] = mock.calls[k] - (before[k] || 0); });
  return delta;
}
out.host_calls = callsOf(false);
out.device_calls = callsOf(true);
NEW.forEach(function (k) { check(!(k in out.host_calls), 'the default hand-off called ' + k); });
check(!('camshiftInitPairs' in out.device_calls) && !('camshiftInitBound' in out.device_calls), 'the device hand-off initialised trackers from the host');
check(out.device_calls.camshiftInitBest === 2 && out.device_calls.camshiftInitBestResult === 2, 'one camshiftInitBest and one result per detect step');

{
  mock.withInitBest(false);
  const before = JSON.stringify(mock.calls);
  let threw = false;
  try { new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, grouping: 'device', handoff: 'device' }); } catch (e) { threw = !(e instanceof RangeError) && /camshiftInitBest/.test(e.message); }
  if (check(threw, "handoff: 'device' on an addon without the calls must throw")) out.missing_checks++;
  if (check(JSON.stringify(mock.calls) === before, 'the refused DeviceBatch reached the addon')) out.missing_checks++;
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, grouping: 'device' }); /* the host hand-off needs neither */
  b.upload(new Uint8Array(fs.readFileSync(job.frames)), 0);
  if (check(b.detectStep(0, 1).rects.length === 4 * job.n, 'host hand-off on an addon without the calls')) out.missing_checks++;
  b.destroy();
  mock.withInitBest(true);
}
console.log(JSON.stringify(out));
