'use strict';
/* GPU run of the JavaScript layer of the per-face initTracker (driven by tests/test_gpu_init_faces.py):
 *     node tests/js/init_faces_gpu.js job.json
 * tests/js/init_faces_common.js on the PRODUCT addon: ccv.DeviceBatch.initFaces / initFacesResult against the records the Python
 * restatement expects; then the raw addon calls' refusals.  Prints one JSON line and leaves through exitNow (contexts destroyed while the
 * HIP runtime is up). */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const pack = require(path.join(root, 'headtrackr_amd', 'js', 'cascade_pack.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], compared: 0, refusals: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }

try {
  require(path.join(__dirname, 'init_faces_common.js'))(headtrackr, job, out, check);

  check(A.CSF_ASSOCIATE === 1 && A.CSF_MAX_SLOTS === 16, 'CSF constants');
  const frames = new Uint8Array(fs.readFileSync(job.frames));
  const ctx = A.createContext({ cascade: pack.packCascade(headtrackr.cascade), interval: 5, device: 0 });
  A.setGeometry(ctx, job.w, job.h, job.n, null);
  A.upload(ctx, frames, job.n, job.w, job.h);
  A.camshiftReserve(ctx, job.trackers);
  const pairs = Int32Array.from(job.calls[0].pairs), np = pairs.length >> 1;
  const refused = function (what, status, fn) { let ok = false; try { fn(); } catch (e) { ok = e.message.indexOf('status ' + status) >= 0; } if (check(ok, what + ' must be refused with status ' + status)) out.refusals++; };
  refused('camshiftInitFaces without a device-grouped batch', -6, function () { A.camshiftInitFaces(ctx, pairs, -10, 0); });
  refused('camshiftInitFacesResult without a call', -6, function () { A.camshiftInitFacesResult(ctx, np); });
  A.detectEnqueue(ctx, A.INPUT_RGBA);
  A.detectBestEnqueue(ctx, 1, 0);
  refused('a NaN threshold', -1, function () { A.camshiftInitFaces(ctx, pairs, NaN, 0); });
  refused('an unknown flag bit', -1, function () { A.camshiftInitFaces(ctx, pairs, -10, 2); });
  const many = new Int32Array(2 * 17);
  for (let i = 0; i < 17; i++) { many[2 * i] = i; many[2 * i + 1] = 0; }
  refused('17 slots on one frame', -1, function () { A.camshiftInitFaces(ctx, many, -10, 0); });
  A.camshiftInitFaces(ctx, pairs, job.calls[0].minConfidence); /* flags left out: rank order */
  const rec = A.camshiftInitFacesResult(ctx, np);
  check(rec instanceof Int32Array && rec.length === 8 * np, 'camshiftInitFacesResult shape');
  if (!job.calls[0].associate) for (let i = 0; i < 8 * np; i++) if (!check(rec[i] === job.calls[0].expect[i], 'raw call: record word ' + i)) break;
  refused('camshiftInitFacesResult with another n', -6, function () { A.camshiftInitFacesResult(ctx, np + 1); });
  A.collectBestDevice(ctx, -1);
  A.destroy(ctx);
} catch (e) {
  check(false, 'exception: ' + (e && e.stack ? e.stack : e));
}
console.log(JSON.stringify(out));
A.exitNow(out.ok ? 0 : 1);
