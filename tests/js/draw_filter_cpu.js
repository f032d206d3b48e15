'use strict';
/* CPU-side checks of the prefiltered draw list's JavaScript layer (driven by tests/test_draw_filter_cpu.py; no GPU):
 *     node tests/js/draw_filter_cpu.js job.json
 * job: { w, h, prefilters: [..], feeds: [{file (one packed frame), width, height, format, matrix, rect | null}] }
 *  1. ccv.DeviceBatch with mixed opts.sources on tests/js/mock_addon_draw_filter.js: drawList / drawListBound WITHOUT opts (and with {} and
 *     {prefilter: null}) issue exactly today's drawListDevice call, before and after the filtered ones; with opts.prefilter they issue ONE
 *     drawListFilteredDevice call and no other draw.  The CRC-32 of every canvas and the factors are printed; Python compares them with the
 *     restatement.  drawList waits only when depth > 1, as the plain call does.
 *  2. malformed opts and opts.prefilter throw; an addon without drawListFilteredDevice gives the "rebuild it" error for opts.prefilter only.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_draw_filter.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], plain: [], filtered: [], refusals: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function snapshot() { return Object.assign({}, mock.calls); }
function called(before) { /* the draw entry points taken since `before` */
  const res = [];
  Object.keys(mock.calls).sort().forEach(function (k) { const d = mock.calls[k] - (before[k] || 0); if (d && /^draw/.test(k)) res.push(d === 1 ? k : k + ' x' + d); });
  return res;
}
function throwsLike(fn, re, what) { let ok = false; try { fn(); } catch (e) { ok = re.test(e.message); if (!ok) out.errors.push(what + ': threw "' + e.message + '"'); } if (check(ok, what)) out.refusals++; }

mock.withIngest(true); mock.withYuv(true); mock.withDrawList(true); mock.withDrawFilter(true);
const n = job.feeds.length, fb = job.w * job.h * 4;
const sources = job.feeds.map(function (f) { const s = { width: f.width, height: f.height, sets: 1, format: f.format }; if (f.format !== 'rgba') s.matrix = f.matrix; return s; });
const rects = job.feeds.map(function (f, i) { return f.rect ? ((i & 1) ? f.rect : Int32Array.from(f.rect)) : null; });
const frames = job.feeds.map(function (f) { return new Uint8Array(fs.readFileSync(f.file)); });

[1, 2].forEach(function (depth) {
  mock.traceReset();
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: depth, sets: 2, sources: sources });
  frames.forEach(function (fr, i) { db.uploadSourceOf(i, fr); });
  const set = mock.trace.devs[0], c0 = mock.trace.ctxs[0];
  const ofSet = function (k) { const r = []; for (let i = 0; i < n; i++) r.push(crc32(set.buf.subarray(k * n * fb + i * fb, k * n * fb + (i + 1) * fb))); return r; };
  const ofBound = function () { const r = []; for (let i = 0; i < n; i++) r.push(crc32(c0.frames.subarray(i * fb, (i + 1) * fb))); return r; };
  const plainRound = function (o, how) {
    let b = snapshot();
    if (how === 'absent') db.drawList(0, 1, rects); else db.drawList(0, 1, rects, o);
    const res = { list: ofSet(1), listCalled: called(b) };
    b = snapshot();
    if (how === 'absent') db.drawListBound(0, rects); else db.drawListBound(0, rects, o);
    res.bound = ofBound(); res.boundCalled = called(b);
    return res;
  };
  const rounds = [plainRound(undefined, 'absent')];
  job.prefilters.forEach(function (mf) {
    set.buf.fill(0xA5);
    let b = snapshot();
    db.drawList(0, 1, rects, { prefilter: mf });
    const res = { depth: depth, prefilter: mf, list: ofSet(1), listCalled: called(b), untouched: set.buf.subarray(0, n * fb).every(function (v) { return v === 0xA5; }) };
    b = snapshot();
    db.drawListBound(0, rects, { prefilter: mf });
    res.bound = ofBound(); res.boundCalled = called(b);
    const wb = db.whitebalance(-1); /* the bound filtered frames feed the step functions */
    res.stepped = wb.length === n;
    b = snapshot();
    res.factors = Array.from(db.drawFilterFactors(rects, { prefilter: mf }));
    res.factorsCalled = called(b);
    out.filtered.push(res);
  });
  rounds.push(plainRound({}, 'empty'), plainRound({ prefilter: null }, 'null'), plainRound({ prefilter: undefined }, 'undefined'));
  rounds.forEach(function (r) { r.depth = depth; out.plain.push(r); });
  throwsLike(function () { db.drawList(0, 1, rects, { prefilter: 0 }); }, /opts\.prefilter is an integer 1\.\.8/, 'prefilter 0 throws');
  throwsLike(function () { db.drawList(0, 1, rects, { prefilter: 9 }); }, /opts\.prefilter is an integer 1\.\.8/, 'prefilter 9 throws');
  throwsLike(function () { db.drawListBound(0, rects, { prefilter: 2.5 }); }, /opts\.prefilter is an integer 1\.\.8/, 'a fractional prefilter throws');
  throwsLike(function () { db.drawListBound(0, rects, { prefilter: '8' }); }, /opts\.prefilter is an integer 1\.\.8/, 'a string prefilter throws');
  throwsLike(function () { db.drawList(0, 1, rects, 8); }, /opts is an object/, 'opts that is a number throws');
  throwsLike(function () { db.drawFilterFactors(rects, {}); }, /opts\.prefilter is an integer 1\.\.8/, 'drawFilterFactors without a prefilter throws');
  throwsLike(function () { db.drawList(0, 1, rects.map(function (r, i) { return i === 2 ? [0, 0, job.feeds[2].width + 1, 1] : null; }), { prefilter: 8 }); }, /entry 2/,
             'a rect outside its source is refused by the addon, naming the entry');
  mock.withDrawFilter(false);
  throwsLike(function () { db.drawList(0, 1, rects, { prefilter: 8 }); }, /no drawListFilteredDevice \(rebuild it\)/, 'an addon without drawListFilteredDevice gives the rebuild-it error');
  throwsLike(function () { db.drawListBound(0, rects, { prefilter: 1 }); }, /no drawListFilteredDevice \(rebuild it\)/, 'the same for drawListBound, at prefilter 1 too');
  const b = snapshot();
  db.drawList(0, 1, rects); /* ... and the plain call does not need it */
  check(called(b).join() === (depth > 1 ? 'drawListDevice,drawListDeviceWaited' : 'drawListDevice'), 'depth ' + depth + ': the plain call works on an addon without the filtered one');
  mock.withDrawFilter(true);
  db.destroy();
});

process.stdout.write(JSON.stringify(out) + '\n');
