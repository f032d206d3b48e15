'use strict';
/* CPU-side checks of the draw list's JavaScript layer (driven by tests/test_draw_list_cpu.py; no GPU):
 *     node tests/js/draw_list_cpu.js job.json
 * job: { w, h, feeds: [{file (one packed frame), width, height, format, matrix, rect | null}], rgba: {file, w, h} }
 *  1. ccv.DeviceBatch with mixed opts.sources: uploadSourceOf + drawList into a frame set, then the set read back from the mock's device buffer — the CRC-32 of every canvas is printed, Python compares it
 *     with the numpy / oracle expectation; drawListBound + whitebalance(-1) equals getWhitebalance of the drawn canvases; only
 *     drawListDevice is logged, never a single-source draw; drawList waits only when depth > 1;
 *  2. malformed opts.sources and malformed rects throw; opts.sources with opts.source throws; an addon without drawListDevice gives the
 *     "rebuild it" error;
 *  3. an RGBA opts.source batch still logs drawFramesDevice.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_draw_list.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], list_crc: [], bound_crc: [], list_checks: 0, refusals: 0, rgba_checks: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function calls(k) { return mock.calls[k] || 0; }
function throwsLike(fn, re, what) { let ok = false; try { fn(); } catch (e) { ok = re.test(e.message); if (!ok) out.errors.push(what + ': threw "' + e.message + '"'); } if (check(ok, what)) out.refusals++; }

mock.withIngest(true); mock.withYuv(true); mock.withDrawList(true);
const n = job.feeds.length, fb = job.w * job.h * 4;
const sources = job.feeds.map(function (f, i) { const s = { width: f.width, height: f.height, sets: 2 }; if (f.format !== 'rgba' || (i & 1)) s.format = f.format; if (f.format !== 'rgba') s.matrix = f.matrix; return s; });
const rects = job.feeds.map(function (f, i) { return f.rect ? ((i & 1) ? f.rect : Int32Array.from(f.rect)) : null; });
const frames = job.feeds.map(function (f) { return new Uint8Array(fs.readFileSync(f.file)); });

/* 1. drawList / drawListBound on mixed feeds */
[1, 2].forEach(function (depth) {
  const before = { list: calls('drawListDevice'), rgba: calls('drawFramesDevice'), yuv: calls('drawFramesYuvDevice'), waited: calls('drawListDeviceWaited') };
  mock.traceReset();
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: depth, sets: 2, sources: sources });
  frames.forEach(function (fr, i) { db.uploadSourceOf(i, fr, 1); });
  db.drawList(1, 1, rects);
  check(calls('drawListDeviceWaited') - before.waited === (depth > 1 ? 1 : 0), 'depth ' + depth + ': drawList waits only when depth > 1');
  const wb = db.whitebalance(1);
  const canv = [];
  db.drawListBound(1, rects);
  const wbb = db.whitebalance(-1);
  const c0 = mock.trace.ctxs[0]; /* context 0's own frames, as the mock keeps them */
  for (let i = 0; i < n; i++) canv.push(c0.frames.subarray(i * fb, (i + 1) * fb));
  if (depth === 1) canv.forEach(function (p) { out.bound_crc.push(crc32(p)); });
  let ok = true;
  for (let i = 0; i < n; i++) {
    const want = headtrackr.getWhitebalance(new Canvas(job.w, job.h).setFrame(Uint8Array.from(canv[i])));
    ok = ok && wb[i] === want && wbb[i] === want;
  }
  if (check(ok, 'depth ' + depth + ': whitebalance of the drawn set and of the bound frames')) out.list_checks++;
  const r = db.detectStep(-1);
  if (check(r.best.length === 6 * n, 'depth ' + depth + ': detectStep on the bound drawn frames')) out.list_checks++;
  if (check(calls('drawListDevice') === before.list + 2 && calls('drawFramesDevice') === before.rgba && calls('drawFramesYuvDevice') === before.yuv,
            'depth ' + depth + ': the facade must take drawListDevice and no single-source draw')) out.list_checks++;
  db.drawList(1, 0, null); /* whole sources */
  throwsLike(function () { db.drawList(1, 0, rects.slice(1)); }, /rects is null or an array/, 'a rects array of the wrong length throws');
  throwsLike(function () { db.drawList(1, 0, rects.map(function () { return [0, 0, 4]; })); }, /rects\[0\]/, 'a rect of three numbers throws');
  throwsLike(function () { db.drawListBound(1, rects.map(function () { return [0, 0.5, 4, 4]; })); }, /rects\[0\]/, 'a rect with a fraction throws');
  throwsLike(function () { db.drawList(1, 0, 'all'); }, /rects is null or an array/, 'rects of another type throws');
  throwsLike(function () { db.drawList(2, 0, null); }, /source set/, 'a source set the feeds do not have throws');
  throwsLike(function () { db.uploadSourceOf(n, frames[0], 0); }, /feed/, 'uploadSourceOf of a feed that does not exist throws');
  throwsLike(function () { db.uploadSourceOf(0, frames[0].subarray(0, frames[0].length - 1), 0); }, /bytes/, 'uploadSourceOf of too few bytes throws');
  throwsLike(function () { db.drawList(1, 0, rects.map(function (r, i) { return i === 2 ? [0, 0, job.feeds[2].width + 1, 1] : null; })); }, /entry 2/, 'a rect outside its source is refused by the addon, naming the entry');
  throwsLike(function () { db.uploadSource(frames[0], 0); }, /opts\.source/, 'uploadSource on a batch with opts.sources throws');
  db.destroy();
});
/* the canvases drawList wrote into set 1 (depth 1), read from a fresh batch through deviceDownload */
(function () {
  mock.traceReset();
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 2, sources: sources });
  frames.forEach(function (fr, i) { db.uploadSourceOf(i, fr); });
  db.drawList(0, 1, rects);
  const set = mock.trace.devs[0]; /* the frame-set buffer: set 1 begins n frames in */
  for (let i = 0; i < n; i++) out.list_crc.push(crc32(set.buf.subarray(n * fb + i * fb, n * fb + (i + 1) * fb)));
  db.destroy();
})();

/* 2. malformed opts.sources */
const mk = function (o) { return function () { return new headtrackr.ccv.DeviceBatch(job.w, job.h, n, Object.assign({ depth: 1, sets: 1 }, o)); }; };
throwsLike(mk({ sources: sources, source: { width: 8, height: 8, sets: 1 } }), /opts\.sources together with opts\.source/, 'opts.sources with opts.source throws');
throwsLike(mk({ sources: sources.slice(1) }), /one entry per feed/, 'a sources list of the wrong length throws');
throwsLike(mk({ sources: { width: 8, height: 8 } }), /one entry per feed/, 'sources that is no array throws');
throwsLike(mk({ sources: sources.map(function (s, i) { return i ? s : null; }) }), /opts\.sources\[0\]/, 'a null source throws');
throwsLike(mk({ sources: sources.map(function (s, i) { return i ? s : { width: 0, height: 8 }; }) }), /width and height/, 'a source without a size throws');
throwsLike(mk({ sources: sources.map(function (s, i) { return i ? s : { width: 8, height: 8, format: 'nv21' }; }) }), /format/, 'an unknown format name throws');
throwsLike(mk({ sources: sources.map(function (s, i) { return i ? s : { width: 8, height: 8, format: 'nv12', matrix: 'bt2020' }; }) }), /matrix/, 'an unknown matrix name throws');
throwsLike(mk({ sources: sources.map(function (s, i) { return i ? s : { width: 8, height: 8, sets: 0 }; }) }), /sets/, 'sets = 0 throws');
mock.withDrawList(false);
throwsLike(mk({ sources: sources }), /no drawListDevice \(rebuild it\)/, 'an addon without drawListDevice gives the rebuild-it error');
mock.withDrawList(true);

/* 3. RGBA opts.source stays on the old entry point */
(function () {
  const g = job.rgba, bytes = new Uint8Array(fs.readFileSync(g.file));
  const l0 = calls('drawListDevice'), r0 = calls('drawFramesDevice');
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, 1, { depth: 1, sets: 1, source: { width: g.w, height: g.h, sets: 1 } });
  db.uploadSource(bytes, 0);
  db.draw(0, 0);
  if (check(calls('drawFramesDevice') === r0 + 1 && calls('drawListDevice') === l0, 'an RGBA opts.source batch must log the old entry point')) out.rgba_checks++;
  throwsLike(function () { db.drawList(0, 0, null); }, /opts\.sources/, 'drawList on a batch without opts.sources throws');
  db.destroy();
})();

process.stdout.write(JSON.stringify(out) + '\n');
