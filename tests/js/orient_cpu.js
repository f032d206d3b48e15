'use strict';
/* The orientation of a feed in the JavaScript layer, on tests/js/mock_addon_422.js (driven by tests/test_orient_bindings_cpu.py; no GPU):
 *     node tests/js/orient_cpu.js
 * ccv.drawFrames videos and ccv.DeviceBatch sources take `orientation` = 0..7 and the facade packs it into the format number it already
 * passes (format | k << 8).  The mock's drawFramesYuvDevice and drawListDevice are wrapped: every format number that reaches the addon is
 * recorded, then the call is handed on with the bits cleared (the mock knows no orientation; what is drawn is not looked at here).
 * Prints one JSON line. */
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_422.js'));
mock.install();
mock.withIngest(true); mock.withYuv(true); mock.withDrawList(true);
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));
const out = { yuv: [], lists: [], thrown: [], factors: null };
const yuvDraw = mock.drawFramesYuvDevice, listDraw = mock.drawListDevice;
let inList = false;  /* (the mock's drawListDevice draws its YUV entries through its own drawFramesYuvDevice: not the facade's calls) */
mock.drawFramesYuvDevice = function () { const a = Array.from(arguments); if (!inList) out.yuv.push(a[6]); a[6] &= 0xff; return yuvDraw.apply(this, a); };
mock.drawListDevice = function () {
  const a = Array.from(arguments);
  out.lists.push(a[1].map(function (e) { return e.format; }));
  a[1] = a[1].map(function (e) { return Object.assign({}, e, { format: e.format & 0xff }); });
  inList = true;
  try { return listDraw.apply(this, a); } finally { inList = false; }
};
function bad(what, fn) { try { fn(); out.thrown.push([what, null]); } catch (e) { out.thrown.push([what, e.constructor.name + ': ' + e.message]); } }
const W = 6, H = 4, cw = 3;
const frame = function (fmt) { return new Uint8Array(fmt === 'yuyv' || fmt === 'uyvy' ? 4 * cw * H : W * H + 2 * cw * 2).fill(128); };

/* 1. ccv.drawFrames: every YUV format under an orientation, and none */
[['nv12', 5], ['i420', 1], ['yuyv', 7], ['uyvy', 2], ['nv12', 0], ['i420', undefined]].forEach(function (v) {
  headtrackr.ccv.drawFrames({ width: W, height: H, format: v[0], matrix: 'bt709', data: frame(v[0]), orientation: v[1] }, new Canvas(8, 8), null);
});
[8, -1, 1.5, '1'].forEach(function (k) {
  bad('drawFrames orientation ' + JSON.stringify(k), function () { headtrackr.ccv.drawFrames({ width: W, height: H, format: 'nv12', data: frame('nv12'), orientation: k }, new Canvas(8, 8), null); });
});
bad('drawFrames rgba orientation', function () { headtrackr.ccv.drawFrames(Object.assign(new Canvas(W, H), { orientation: 1 }), new Canvas(8, 8), null); });

/* 2. DeviceBatch sources */
const db = new headtrackr.ccv.DeviceBatch(8, 8, 4, { sources: [{ width: W, height: H, format: 'yuyv', orientation: 3 }, { width: W, height: H, orientation: 6 },
  { width: W, height: H, format: 'nv12', matrix: 'bt601-full', orientation: 4 }, { width: W, height: H, format: 'i420' }] });
db.uploadSourceOf(0, frame('yuyv')); db.uploadSourceOf(1, new Uint8Array(W * H * 4).fill(9)); db.uploadSourceOf(2, frame('nv12')); db.uploadSourceOf(3, frame('i420'));
db.drawListBound(0, null);
/* the sizes drawFilterFactors asks the library about: the whole source of an odd orientation is height x width */
mock.drawFilterFactors = function (sizes) { out.factors = Array.from(sizes); return new Int32Array(sizes.length).fill(1); };
db.drawFilterFactors(null, { prefilter: 8 });
delete mock.drawFilterFactors;
db.destroy();
[8, -1, 0.5].forEach(function (k) {
  bad('DeviceBatch orientation ' + k, function () { new headtrackr.ccv.DeviceBatch(8, 8, 1, { sources: [{ width: W, height: H, format: 'nv12', orientation: k }] }); });
});
console.log(JSON.stringify(out));
