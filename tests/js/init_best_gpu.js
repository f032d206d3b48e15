'use strict';
/* GPU run of the JavaScript layer of the device hand-off (driven by tests/test_gpu_init_best.py):
 *     node tests/js/init_best_gpu.js job.json
 * tests/js/init_best_common.js on the PRODUCT addon: ccv.DeviceBatch with {grouping: 'device', handoff: 'device'} against the default; then
 * the raw addon calls' call-sequence errors.  Prints one JSON line and leaves through exitNow (contexts destroyed while the HIP runtime is up). */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const pack = require(path.join(root, 'headtrackr_amd', 'js', 'cascade_pack.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], compared: 0, range_errors: 0, state_errors: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }

try {
  require(path.join(__dirname, 'init_best_common.js'))(headtrackr, job, out, check);

  const frames = new Uint8Array(fs.readFileSync(job.frames));
  const ctx = A.createContext({ cascade: pack.packCascade(headtrackr.cascade), interval: 5, device: 0 });
  A.setGeometry(ctx, job.w, job.h, job.n, null);
  A.upload(ctx, frames, job.n, job.w, job.h);
  A.camshiftReserve(ctx, job.n);
  const pairs = new Int32Array(2 * job.n);
  for (let f = 0; f < job.n; f++) { pairs[2 * f] = job.n - 1 - f; pairs[2 * f + 1] = f; }
  const refused = function (what, status, fn) { let ok = false; try { fn(); } catch (e) { ok = e.message.indexOf('status ' + status) >= 0; } if (check(ok, what + ' must be refused with status ' + status)) out.state_errors++; };
  refused('camshiftInitBest without a device-grouped batch', -6, function () { A.camshiftInitBest(ctx, pairs, -10, null); });
  refused('camshiftInitBestResult without a call', -6, function () { A.camshiftInitBestResult(ctx, job.n); });
  A.detectEnqueue(ctx, A.INPUT_RGBA);
  A.detectBestEnqueue(ctx, 1, 0);
  refused('a NaN threshold', -1, function () { A.camshiftInitBest(ctx, pairs, NaN, null); });
  A.camshiftInitBest(ctx, pairs, -10); /* fallback left out */
  const res = A.camshiftInitBestResult(ctx, job.n), r = A.collectBestDevice(ctx, -1);
  check(res.codes instanceof Int32Array && res.codes.length === job.n && res.rects instanceof Int32Array && res.rects.length === 4 * job.n, 'camshiftInitBestResult shape');
  for (let f = 0; f < job.n; f++) {
    const face = r.best[6 * f + 5] > 0 && r.best[6 * f + 4] > -10;
    check(res.codes[f] === (face ? A.CSB_FACE : A.CSB_UNTOUCHED), 'code of frame ' + f);
    for (let k = 0; k < 4; k++) check(res.rects[4 * f + k] === (face ? Math.floor(r.best[6 * f + k]) : 0), 'rect of frame ' + f);
  }
  refused('camshiftInitBestResult with another n', -6, function () { A.camshiftInitBestResult(ctx, job.n - 1); });
  A.destroy(ctx);
} catch (e) {
  check(false, 'exception: ' + (e && e.stack ? e.stack : e));
}
console.log(JSON.stringify(out));
A.exitNow(out.ok ? 0 : 1);
