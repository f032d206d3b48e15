'use strict';
/* GPU run of the JavaScript layer of the device grouping (driven by tests/test_gpu_group.py):
 *     node tests/js/group_gpu.js job.json
 * tests/js/group_common.js on the PRODUCT addon: ccv.DeviceBatch with {grouping: 'device'} against the default host route, the CPU oracle's
 * best faces and the reference's recorded grouped rects; then the raw addon calls DeviceBatch does not use (detectBestRecords, groupHits)
 * and the call-sequence errors.  Prints one JSON line and leaves through exitNow (contexts destroyed while the HIP runtime is up). */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const pack = require(path.join(root, 'headtrackr_amd', 'js', 'cascade_pack.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], compared: 0, state_errors: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }

try {
  require(path.join(__dirname, 'group_common.js'))(headtrackr, job, out, check);

  const frames = new Uint8Array(fs.readFileSync(job.frames));
  const ctx = A.createContext({ cascade: pack.packCascade(headtrackr.cascade), interval: 5, device: 0 });
  A.setGeometry(ctx, job.w, job.h, job.n, null);
  const refused = function (what, fn) { let ok = false; try { fn(); } catch (e) { ok = /status -6/.test(e.message); } if (check(ok, what + ' must be refused with HT_ERR_STATE')) out.state_errors++; };
  refused('detectBestEnqueue without a batch', function () { A.detectBestEnqueue(ctx, 1, 0); });
  refused('detectBestRecords without a batch', function () { A.detectBestRecords(ctx); });
  refused('detectGrouped without a batch', function () { A.detectGrouped(ctx, 0); });
  A.upload(ctx, frames, job.n, job.w, job.h);
  A.detectEnqueue(ctx, A.INPUT_RGBA);
  refused('collectBestDevice without detectBestEnqueue', function () { A.collectBestDevice(ctx, -1); });
  A.detectBestEnqueue(ctx, 1, 7);
  const r = A.collectBestDevice(ctx, -1), rec = A.detectBestRecords(ctx);
  check(JSON.stringify(Array.from(r.best)) === JSON.stringify(job.expect_best), 'collectBestDevice differs from the oracle');
  let recOk = rec.length === 8 * job.n;
  for (let f = 0; recOk && f < job.n; f++) {
    for (let k = 0; k < 6; k++) recOk = recOk && Object.is(rec[8 * f + k], r.best[6 * f + k]);
    recOk = recOk && rec[8 * f + 6] === 7 + f && rec[8 * f + 7] === 1;
  }
  check(recOk, 'detectBestRecords: records differ from [best, frameBase + f, 1]');
  /* groupHits: the batch's own raw hits as 24-byte records, frames reversed in arrival order */
  A.detectEnqueue(ctx, A.INPUT_RGBA);
  const h = A.detectCollect(ctx), n = h.sum.length, bytes = new Uint8Array(24 * n), dv = new DataView(bytes.buffer);
  for (let k = 0; k < n; k++) {
    const o = 24 * (n - 1 - k);
    dv.setUint32(o, h.frame[k], true); dv.setUint16(o + 4, h.x[k], true); dv.setUint16(o + 6, h.y[k], true); dv.setUint8(o + 8, h.scale[k]); dv.setUint8(o + 9, h.q[k]);
    dv.setFloat64(o + 16, h.sum[k], true);
  }
  const g = A.groupHits(ctx, bytes, job.n, 1);
  check(JSON.stringify(Array.from(g.best)) === JSON.stringify(job.expect_best), 'groupHits.best differs from the oracle');
  const want = [].concat.apply([], job.expect_grouped.map(function (l) { return l.map(function (q) { return [q.x, q.y, q.width, q.height, q.confidence, q.neighbors]; }); }));
  check(JSON.stringify(Array.from(g.grouped)) === JSON.stringify([].concat.apply([], want)), 'groupHits.grouped differs from the recorded rects');
  check(JSON.stringify(Array.from(g.counts)) === JSON.stringify(job.expect_grouped.map(function (l) { return l.length; })), 'groupHits.counts');
  out.hits = n;
  A.destroy(ctx);
} catch (e) {
  check(false, 'exception: ' + (e && e.stack ? e.stack : e));
}
console.log(JSON.stringify(out));
A.exitNow(out.ok ? 0 : 1);
