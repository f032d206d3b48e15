'use strict';
/* CPU-side checks of the YUV ingest's JavaScript layer (driven by tests/test_ingest_yuv_cpu.py; no GPU):
 *     node tests/js/ingest_yuv_cpu.js job.json
 * job: { cases: [{file (one packed frame), w, h, format, matrix, dw, dh, rect | null}], batch: {file (n packed frames), n, w, h, format,
 *        matrix, dw, dh, expect: [file per frame: the expected canvas, RGBA]}, rgba: {file, w, h, dw, dh} }
 *  1. ccv.drawFrames on a YUV video-like object goes deviceUpload -> drawFramesYuvDevice -> deviceDownload; the CRC-32 of every canvas is
 *     printed (Python compares it with the numpy / oracle expectation);
 *  2. on an addon WITHOUT the call it throws (a canvas cannot draw planes: there is no host route); a bad format / matrix name throws;
 *  3. ccv.DeviceBatch with opts.sourceFormat: uploadSource / draw / drawBound call drawFramesYuvDevice (never drawFramesDevice), draw waits
 *     only when depth > 1, and the step functions see the drawn frames (whitebalance of the drawn set == of the expected canvases);
 *  4. an RGBA video still takes drawFramesDevice, and a DeviceBatch without sourceFormat too.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_yuv.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], canvas_crc: [], device_checks: 0, batch_checks: 0, rgba_checks: 0, refusals: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function calls(k) { return mock.calls[k] || 0; }
const FORMATS = ['nv12', 'i420'], MATRICES = ['bt601', 'bt709', 'bt601-full', 'bt709-full'];

mock.withIngest(true);
mock.withYuv(true);
job.cases.forEach(function (cs, k) {
  const video = { width: cs.w, height: cs.h, format: FORMATS[cs.format], matrix: MATRICES[cs.matrix], data: new Uint8Array(fs.readFileSync(cs.file)) };
  if (cs.matrix === 0 && (k & 1)) delete video.matrix; /* the default is 'bt601' */
  const y0 = calls('drawFramesYuvDevice'), r0 = calls('drawFramesDevice'), d0 = calls('deviceDownload');
  const c = new Canvas(cs.dw, cs.dh);
  c.pixels.fill(77);
  headtrackr.ccv.drawFrames(video, c, cs.rect || undefined);
  out.canvas_crc.push(crc32(c.pixels));
  if (check(calls('drawFramesYuvDevice') === y0 + 1 && calls('drawFramesDevice') === r0 && calls('deviceDownload') === d0 + 1, 'case ' + k + ': the YUV device route was not taken')) out.device_checks++;
});

/* 2. refusals */
(function () {
  const cs = job.cases[0], data = new Uint8Array(fs.readFileSync(cs.file));
  const attempt = function (video, re, what) {
    let threw = false;
    try { headtrackr.ccv.drawFrames(video, new Canvas(cs.dw, cs.dh)); } catch (e) { threw = re.test(e.message); }
    if (check(threw, what)) out.refusals++;
  };
  attempt({ width: cs.w, height: cs.h, format: 'nv21', data: data }, /format/, 'an unknown format name throws');
  attempt({ width: cs.w, height: cs.h, format: 'nv12', matrix: 'bt2020', data: data }, /matrix/, 'an unknown matrix name throws');
  attempt({ width: cs.w, height: cs.h, format: 'nv12', data: data.subarray(0, data.length - 1) }, /video\.data/, 'short data throws');
  mock.withYuv(false);
  attempt({ width: cs.w, height: cs.h, format: 'nv12', data: data }, /drawFramesYuvDevice/, 'an addon without the call throws');
  let threw = false;
  try { new headtrackr.ccv.DeviceBatch(cs.dw, cs.dh, 1, { depth: 1, source: { width: cs.w, height: cs.h, sets: 1 }, sourceFormat: 'nv12' }); } catch (e) { threw = /drawFramesYuvDevice/.test(e.message); }
  if (check(threw, 'DeviceBatch with sourceFormat on an addon without the call throws')) out.refusals++;
  mock.withYuv(true);
})();

/* 3. DeviceBatch with a YUV source buffer */
(function () {
  const b = job.batch, frames = new Uint8Array(fs.readFileSync(b.file));
  const want = b.expect.map(function (f) { return headtrackr.getWhitebalance(new Canvas(b.dw, b.dh).setFrame(new Uint8Array(fs.readFileSync(f)))); });
  [1, 2].forEach(function (depth) {
    const r0 = calls('drawFramesDevice');
    const db = new headtrackr.ccv.DeviceBatch(b.dw, b.dh, b.n, { depth: depth, sets: 2, source: { width: b.w, height: b.h, sets: 2 }, sourceFormat: FORMATS[b.format], sourceMatrix: MATRICES[b.matrix] });
    db.uploadSource(frames, 1);
    const waited = calls('drawFramesYuvDeviceWaited');
    db.draw(1, 1);
    check((calls('drawFramesYuvDeviceWaited') - waited) === (depth > 1 ? 1 : 0), 'depth ' + depth + ': draw waits only when depth > 1');
    const wb = db.whitebalance(1);
    let ok = true;
    for (let f = 0; f < b.n; f++) ok = ok && wb[f] === want[f];
    if (check(ok, 'depth ' + depth + ': whitebalance of the drawn set')) out.batch_checks++;
    db.drawBound(1);
    const r = db.detectStep(-1);
    if (check(r.best.length === 6 * b.n, 'depth ' + depth + ': detectStep on the bound drawn frames')) out.batch_checks++;
    check(calls('drawFramesDevice') === r0, 'depth ' + depth + ': a YUV batch reached the RGBA entry point');
    let threw = false;
    try { db.uploadSource(frames.subarray(0, frames.length - 1), 0); } catch (e) { threw = e instanceof RangeError; }
    check(threw, 'uploadSource of too few bytes throws');
    db.destroy();
  });
})();

/* 4. RGBA stays RGBA */
(function () {
  const g = job.rgba, bytes = new Uint8Array(fs.readFileSync(g.file));
  const video = new Canvas(g.w, g.h).setFrame(bytes);
  const y0 = calls('drawFramesYuvDevice'), r0 = calls('drawFramesDevice');
  const c = headtrackr.ccv.drawFrames(video, new Canvas(g.dw, g.dh));
  out.rgba_crc = crc32(c.pixels);
  if (check(calls('drawFramesDevice') === r0 + 1 && calls('drawFramesYuvDevice') === y0, 'an RGBA video must log the RGBA entry point')) out.rgba_checks++;
  const db = new headtrackr.ccv.DeviceBatch(g.dw, g.dh, 1, { depth: 1, sets: 1, source: { width: g.w, height: g.h, sets: 1 } });
  db.uploadSource(bytes, 0);
  db.draw(0, 0);
  if (check(calls('drawFramesDevice') === r0 + 2 && calls('drawFramesYuvDevice') === y0, 'an RGBA batch must log the RGBA entry point')) out.rgba_checks++;
  db.destroy();
})();

process.stdout.write(JSON.stringify(out) + '\n');
