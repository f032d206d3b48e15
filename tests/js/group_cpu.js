'use strict';
/* CPU-side checks of the JavaScript layer of the device grouping (driven by tests/test_group_cases_cpu.py; no GPU):
 *     node tests/js/group_cpu.js job.json
 *  1. tests/js/group_common.js on the oracle-backed mock addon (tests/js/mock_addon_group.js): {grouping: 'device'} returns what the
 *     default route returns — the expectations of the GPU run (tests/js/group_gpu.js);
 *  2. the default route makes none of the new addon calls, the device route none of collectBest / detectCollect;
 *  3. on an addon without the new calls (withGroup(false)) {grouping: 'device'} throws an Error that names what is missing before anything
 *     reaches the addon; an unknown grouping is a RangeError.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_group.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], compared: 0, host_calls: null, device_calls: null, missing_checks: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const NEW = ['detectBestEnqueue', 'collectBestDevice', 'detectGrouped', 'detectBestRecords', 'groupHits'];

require(path.join(__dirname, 'group_common.js'))(headtrackr, job, out, check);

/* 2. which addon calls each route makes */
function callsOf(grouping) {
  const before = Object.assign({}, mock.calls), delta = {};
  const o = { depth: 2 };
  if (grouping) o.grouping = grouping;
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, o);
  b.upload(new Uint8Array(fs.readFileSync(job.frames)), 0);
  b.detectBest(3, 1, 0); b.detect(1, 0); b.whitebalance(0); b.detectStep(0, 1); b.trackStep(0, true);
  b.destroy();
  Object.keys(mock.calls).forEach(function (k) { if (mock.calls[k] !== (before[k] || 0)) delta[k] = mock.calls[k] - (before[k] || 0); });
  return delta;
}
out.host_calls = callsOf(undefined);
out.device_calls = callsOf('device');
NEW.forEach(function (k) { check(!(k in out.host_calls), 'the default route called ' + k); });
check(!('collectBest' in out.device_calls) && !('detectCollect' in out.device_calls), 'the device route fell back to a host-route call');

/* 3. an addon without the new calls; an unknown option value */
{
  mock.withGroup(false);
  const before = JSON.stringify(mock.calls);
  let threw = false;
  try { new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, grouping: 'device' }); } catch (e) { threw = /detectBestEnqueue/.test(e.message); }
  if (check(threw, "grouping: 'device' on an addon without the calls must throw")) out.missing_checks++;
  if (check(JSON.stringify(mock.calls) === before, 'the refused DeviceBatch reached the addon')) out.missing_checks++;
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1 }); /* the default route needs none of them */
  b.upload(new Uint8Array(fs.readFileSync(job.frames)), 0);
  if (check(b.detectBest(1, 1, 0).best.length === 6 * job.n, 'default route on an addon without the calls')) out.missing_checks++;
  b.destroy();
  mock.withGroup(true);
  threw = false;
  try { new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { grouping: 'gpu' }); } catch (e) { threw = e instanceof RangeError; }
  if (check(threw, 'an unknown grouping must be a RangeError')) out.missing_checks++;
}
console.log(JSON.stringify(out));
