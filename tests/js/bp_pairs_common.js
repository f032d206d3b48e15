'use strict';
/* The JavaScript side of the back-projection-over-pairs tests, shared by tests/js/bp_pairs_cpu.js (oracle-backed mock addon) and
 * tests/js/bp_pairs_gpu.js (product addon on a GPU).
 * job: { cases: [{name, w, h, rects[[4]], frames[raw files], trackers[[{frame, crc, pdf[[x, y, value]]}]]}] } — the recording of the
 * reference (tests/golden/multitrack_bp.json) plus the frames.
 * camshift.MultiTracker.getBackProjectionImgs() after every track(): CRC-32 of every tracker's ImageData against the reference's,
 * getPdf(i) at the recorded points.  `full`: additionally everything against M camshift.Tracker instances on the same canvases, byte for
 * byte, and getBackProjectionImg(i).  counters() -> number of camshiftBackProjectPairs calls so far. */
const fs = require('fs');

const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function sameBytes(x, y) {
  if (x.length !== y.length) return false;
  for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) return false;
  return true;
}
function samePdf(a, b) { /* [x][y] arrays; Object.is distinguishes nothing that matters here (no NaN, no -0) but is the strictest equality */
  if (a.length !== b.length) return false;
  for (let x = 0; x < a.length; x++) {
    if (a[x].length !== b[x].length) return false;
    for (let y = 0; y < a[x].length; y++) if (!Object.is(a[x][y], b[x][y])) return false;
  }
  return true;
}

module.exports = function run(headtrackr, Canvas, job, out, check, counters, opts) {
  const full = !!(opts && opts.full), device = !(opts && opts.device === false);
  job.cases.forEach(function (g) {
    const canvasOf = function (file) { return new Canvas(g.w, g.h).setFrame(fs.readFileSync(file)); };
    const rects = g.rects.map(function (r) { return new headtrackr.camshift.Rectangle(r[0], r[1], r[2], r[3]); });
    const m = rects.length;
    const mt = new headtrackr.camshift.MultiTracker({ calcAngles: true });
    const singles = full ? rects.map(function () { return new headtrackr.camshift.Tracker({ calcAngles: true }); }) : [];
    const c0 = canvasOf(g.frames[0]);
    mt.initTracker(c0, rects);
    singles.forEach(function (t, j) { t.initTracker(c0, rects[j]); });
    check(mt.getBackProjectionImgs() === undefined && mt.getPdf(0) === undefined, g.name + ': nothing to project before the first track()');
    for (let k = 1; k < g.frames.length; k++) {
      const cv = canvasOf(g.frames[k]);
      mt.track(cv);
      singles.forEach(function (t) { t.track(cv); });
      let before = counters();
      const imgs = mt.getBackProjectionImgs();
      check(counters() - before === (device ? 1 : 0), g.name + ' call ' + k + ': getBackProjectionImgs made ' + (counters() - before) + ' device calls');
      out.imgs_calls++;
      check(Array.isArray(imgs) && imgs.length === m, g.name + ': one ImageData per tracker');
      for (let j = 0; j < m; j++) {
        const rec = g.trackers[j][k - 1], img = imgs[j];
        check(img.width === g.w && img.height === g.h && img.data.length === 4 * g.w * g.h, g.name + ': ImageData shape');
        if (check(crc32(img.data) === rec.crc, g.name + ' tracker ' + j + ' call ' + k + ': CRC of getBackProjectionImgs()[j]')) out.crc_checks++;
        before = counters();
        const pdf = mt.getPdf(j);
        check(counters() - before === (device ? 1 : 0), g.name + ': getPdf(i) is one device call');
        check(pdf.length === g.w && pdf[0].length === g.h, g.name + ': getPdf(i) is [x][y]');
        let ok = true;
        rec.pdf.forEach(function (s) { ok = check(Object.is(pdf[s[0]][s[1]], s[2]), g.name + ' tracker ' + j + ' call ' + k + ': pdf[' + s[0] + '][' + s[1] + '] ' + pdf[s[0]][s[1]] + ' != ' + s[2]) && ok; });
        if (ok) out.pdf_checks++;
        if (full) {
          const one = mt.getBackProjectionImg(j);
          check(sameBytes(one.data, img.data), g.name + ' tracker ' + j + ' call ' + k + ': getBackProjectionImg(i) != getBackProjectionImgs()[i]');
          check(sameBytes(singles[j].getBackProjectionImg().data, img.data), g.name + ' tracker ' + j + ' call ' + k + ': differs from camshift.Tracker.getBackProjectionImg()');
          if (check(samePdf(singles[j].getPdf(), pdf), g.name + ' tracker ' + j + ' call ' + k + ': differs from camshift.Tracker.getPdf()')) out.single_checks++;
        }
      }
      /* the trackers are untouched by the getters */
      if (full) singles.forEach(function (t, j) {
        const a = t.getSearchWindow(), b = mt.getSearchWindow(j);
        check(a.x === b.x && a.y === b.y && a.width === b.width && a.height === b.height, g.name + ' tracker ' + j + ' call ' + k + ': search windows');
      });
    }
    let threw = false;
    try { mt.getPdf(m); } catch (e) { threw = e instanceof RangeError; }
    check(threw, g.name + ': getPdf(count()) is a RangeError');
    mt.release();
    singles.forEach(function (t) { t.release(); });
  });
};
module.exports.crc32 = crc32;
