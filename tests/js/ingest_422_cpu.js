'use strict';
/* CPU-side checks of the packed 4:2:2 formats in the JavaScript layer (driven by tests/test_ingest_422_js_cpu.py; no GPU):
 *     node tests/js/ingest_422_cpu.js job.json
 * job: { w, h, sw, sh, videos: [{file (one packed frame), format, matrix, rect | null}] }
 *  1. ccv.drawFrames on {width, height, format: 'yuyv' | 'uyvy', matrix, data}: the canvas's CRC-32 is printed, Python compares it with
 *     tests/yuv422_cases.py; the upload is 4 * ceil(w / 2) * h bytes, one byte less throws;
 *  2. ccv.DeviceBatch with sourceFormat 'yuyv' (uploadSource + drawBound) and with mixed sources [yuyv, rgba, uyvy] (uploadSourceOf +
 *     drawListBound): getWhitebalance of the canvases drawn in 1 equals whitebalance(-1) of the bound frames;
 *  3. an unknown format name throws a RangeError naming the legal ones.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_422.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], crc: [], refusals: 0, batch_checks: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function throwsLike(fn, type, re, what) { let ok = false; try { fn(); } catch (e) { ok = e instanceof type && re.test(e.message); if (!ok) out.errors.push(what + ': threw "' + e.message + '"'); } if (check(ok, what)) out.refusals++; }
mock.withIngest(true); mock.withYuv(true); mock.withDrawList(true);
const bytes = 4 * ((job.sw + 1) >> 1) * job.sh;
const frames = job.videos.map(function (v) { return new Uint8Array(fs.readFileSync(v.file)); });

/* 1. ccv.drawFrames */
const wbs = [];
job.videos.forEach(function (v, i) {
  check(frames[i].length === bytes, 'a packed frame is 4 * ceil(w / 2) * h bytes');
  const canvas = new Canvas(job.w, job.h), before = mock.calls.drawFramesYuvDevice || 0;
  headtrackr.ccv.drawFrames({ width: job.sw, height: job.sh, format: v.format, matrix: v.matrix, data: frames[i] }, canvas, v.rect);
  check((mock.calls.drawFramesYuvDevice || 0) === before + 1, 'video ' + i + ': ONE drawFramesYuvDevice');
  out.crc.push(crc32(canvas.getContext('2d').getImageData(0, 0, job.w, job.h).data));
  wbs.push(v.rect ? null : headtrackr.getWhitebalance(canvas));
  throwsLike(function () { headtrackr.ccv.drawFrames({ width: job.sw, height: job.sh, format: v.format, matrix: v.matrix, data: frames[i].subarray(0, bytes - 1) }, canvas, null); }, RangeError, /bytes/, 'video ' + i + ': one byte short');
});
throwsLike(function () { headtrackr.ccv.drawFrames({ width: job.sw, height: job.sh, format: 'yvyu', data: frames[0] }, new Canvas(job.w, job.h), null); }, RangeError, /format.*'yuyv'.*'uyvy'/, 'unknown format name in drawFrames');

/* 2. DeviceBatch */
const whole = job.videos.findIndex(function (v) { return v.format === 'yuyv' && !v.rect; }), wholeU = job.videos.findIndex(function (v) { return v.format === 'uyvy' && !v.rect; });
if (check(whole >= 0 && wholeU >= 0, 'the job holds a whole-frame video of each format')) {
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, 2, { source: { width: job.sw, height: job.sh }, sourceFormat: 'yuyv', sourceMatrix: job.videos[whole].matrix });
  const two = new Uint8Array(2 * bytes); two.set(frames[whole], 0); two.set(frames[whole], bytes);
  db.uploadSource(two);
  throwsLike(function () { db.uploadSource(two.subarray(0, 2 * bytes - 1)); }, RangeError, /bytes/, 'uploadSource one byte short');
  db.drawBound();
  const wb = db.whitebalance(-1);
  if (check(wb[0] === wbs[whole] && wb[1] === wbs[whole], 'sourceFormat yuyv: the bound frames are the drawn canvas')) out.batch_checks++;
  db.destroy();
  const rgba = mock.toRgba422(frames[whole], 0, job.sw, job.sh, 4, ['bt601', 'bt709', 'bt601-full', 'bt709-full'].indexOf(job.videos[whole].matrix));
  const before = mock.calls.drawListDevice || 0;
  const dm = new headtrackr.ccv.DeviceBatch(job.w, job.h, 3, { sources: [{ width: job.sw, height: job.sh, format: 'yuyv', matrix: job.videos[whole].matrix }, { width: job.sw, height: job.sh },
    { width: job.sw, height: job.sh, format: 'uyvy', matrix: job.videos[wholeU].matrix }] });
  dm.uploadSourceOf(0, frames[whole]); dm.uploadSourceOf(1, rgba); dm.uploadSourceOf(2, frames[wholeU]);
  dm.drawListBound(0, null);
  const wm = dm.whitebalance(-1);
  check((mock.calls.drawListDevice || 0) === before + 1, 'mixed sources: ONE drawListDevice');
  if (check(wm[0] === wbs[whole] && wm[1] === wbs[whole] && wm[2] === wbs[wholeU], 'mixed sources: yuyv, its RGBA conversion and uyvy give the drawn canvases')) out.batch_checks++;
  throwsLike(function () { dm.uploadSourceOf(0, frames[whole].subarray(0, bytes - 1)); }, RangeError, /needs/, 'uploadSourceOf one byte short');
  dm.destroy();
}
/* 3. refusals */
throwsLike(function () { new headtrackr.ccv.DeviceBatch(job.w, job.h, 1, { source: { width: job.sw, height: job.sh }, sourceFormat: 'yuy2' }); }, RangeError, /'nv12', 'i420', 'yuyv' or 'uyvy'/, 'unknown sourceFormat');
throwsLike(function () { new headtrackr.ccv.DeviceBatch(job.w, job.h, 1, { sources: [{ width: 4, height: 4, format: 'vyuy' }] }); }, RangeError, /'yuyv' or 'uyvy'/, 'unknown sources[0].format');
/* (an offset that is no multiple of 4 is the shim's refusal: tests/test_ingest_422_addon_cpu.py has it, on csrc/ht_napi.cc itself) */
console.log(JSON.stringify(out));
