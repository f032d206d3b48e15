'use strict';
/* CPU-side checks of the device drawImage's JavaScript layer (driven by tests/test_ingest_cpu.py; no GPU):
 *     node tests/js/ingest_cpu.js job.json
 * job: { cases: [{file (raw RGBA of sw x sh), sw, sh, dw, dh, rect | null}] }
 *  1. per case the CRC-32 of oracle/canvas_shim.js's resample and of headtrackr_amd/js/canvas.js's drawImage (Python compares both with
 *     its expectation);
 *  2. ccv.drawFrames on an addon WITHOUT the ingest calls (tests/js/mock_addon.js as it is) falls back to the canvas's drawImage: same
 *     bytes, and the addon is not reached;
 *  3. on an addon WITH them (tests/js/mock_addon_ingest.js) it goes deviceUpload -> drawFramesDevice -> deviceDownload: same bytes;
 *  4. ccv.DeviceBatch with opts.source: uploadSource / draw / drawBound call the addon as documented (draw waits only when depth > 1) and
 *     the step functions then see the drawn frames (whitebalance of the drawn set == of the expectation).
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_ingest.js'));
mock.install();
const shim = require(path.join(root, 'oracle', 'canvas_shim.js'));
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], shim_crc: [], canvas_crc: [], fallback_checks: 0, device_checks: 0, batch_checks: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function same(a, b) { if (a.length !== b.length) return false; for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false; return true; }

job.cases.forEach(function (cs, k) {
  const bytes = fs.readFileSync(cs.file), r = cs.rect || [0, 0, cs.sw, cs.sh];
  const want = new Uint8ClampedArray(cs.dw * cs.dh * 4);
  shim.resample(bytes, cs.sw, cs.sh, r[0], r[1], r[2], r[3], want, cs.dw, cs.dh, 0, 0, cs.dw, cs.dh);
  out.shim_crc.push(crc32(want));
  const video = new Canvas(cs.sw, cs.sh).setFrame(bytes);
  const draw = function (target) {
    if (cs.rect) target.getContext('2d').drawImage(video, r[0], r[1], r[2], r[3], 0, 0, cs.dw, cs.dh); else target.getContext('2d').drawImage(video, 0, 0, cs.dw, cs.dh);
    return target;
  };
  out.canvas_crc.push(crc32(draw(new Canvas(cs.dw, cs.dh)).pixels));
  /* 2. an addon without the calls */
  mock.withIngest(false);
  const before = JSON.stringify(mock.calls);
  const c1 = headtrackr.ccv.drawFrames(video, new Canvas(cs.dw, cs.dh), cs.rect || undefined);
  if (check(same(c1.pixels, want), 'case ' + k + ': fallback bytes') && check(JSON.stringify(mock.calls) === before, 'case ' + k + ': the fallback reached the addon')) out.fallback_checks++;
  /* 3. an addon with them */
  mock.withIngest(true);
  const n0 = mock.calls.drawFramesDevice || 0, d0 = mock.calls.deviceDownload || 0;
  const c2 = new Canvas(cs.dw, cs.dh);
  c2.pixels.fill(77);
  headtrackr.ccv.drawFrames(video, c2, cs.rect || undefined);
  if (check(same(c2.pixels, want), 'case ' + k + ': device-route bytes') &&
      check((mock.calls.drawFramesDevice || 0) === n0 + 1 && (mock.calls.deviceDownload || 0) === d0 + 1, 'case ' + k + ': device route not taken')) out.device_checks++;
});

/* 4. DeviceBatch with a source buffer */
(function () {
  const cs = job.cases[job.batch_case], n = 2, bytes = fs.readFileSync(cs.file);
  const two = new Uint8Array(2 * bytes.length);
  two.set(bytes, 0); two.set(bytes.map(function (v) { return 255 - v; }), bytes.length);
  const want = [0, 1].map(function (f) {
    const d = new Uint8ClampedArray(cs.dw * cs.dh * 4);
    shim.resample(two.subarray(f * bytes.length, (f + 1) * bytes.length), cs.sw, cs.sh, 0, 0, cs.sw, cs.sh, d, cs.dw, cs.dh, 0, 0, cs.dw, cs.dh);
    return headtrackr.getWhitebalance(new Canvas(cs.dw, cs.dh).setFrame(d));
  });
  mock.withIngest(true);
  [1, 2].forEach(function (depth) {
    const b = new headtrackr.ccv.DeviceBatch(cs.dw, cs.dh, n, { depth: depth, sets: 2, source: { width: cs.sw, height: cs.sh, sets: 2 } });
    b.uploadSource(two, 1);
    const waited = mock.calls.drawFramesDeviceWaited || 0;
    b.draw(1, 1);
    check(((mock.calls.drawFramesDeviceWaited || 0) - waited) === (depth > 1 ? 1 : 0), 'depth ' + depth + ': draw waits only when depth > 1');
    const wb = b.whitebalance(1);
    if (check(wb[0] === want[0] && wb[1] === want[1], 'depth ' + depth + ': whitebalance of the drawn set')) out.batch_checks++;
    b.drawBound(1);
    const r = b.detectStep(-1);
    check(r.best.length === 6 * n, 'depth ' + depth + ': detectStep on the bound drawn frames');
    const t = b.trackStep(-1, true);
    if (check(t.length === 9 * n, 'depth ' + depth + ': trackStep on the bound drawn frames')) out.batch_checks++;
    b.destroy();
  });
  let threw = false;
  const b0 = new headtrackr.ccv.DeviceBatch(cs.dw, cs.dh, n, { depth: 1 });
  try { b0.draw(0, 0); } catch (e) { threw = /opts\.source/.test(e.message); }
  check(threw, 'draw without opts.source throws');
  b0.destroy();
})();

process.stdout.write(JSON.stringify(out) + '\n');
