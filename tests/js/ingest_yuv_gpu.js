'use strict';
/* The YUV ingest from the JavaScript host, on a GPU (driven by tests/test_gpu_ingest_yuv.py):
 *     node tests/js/ingest_yuv_gpu.js job.json
 * job: { sw, sh, w, h, n, rect, dir, videos: [{file (n packed frames), format, matrix, want, want_rect (n expected canvases each), wb, wb_rect,
 *        best}] } — expectations computed by the declared conversion + the oracle.
 *  1. ccv.drawFrames(video, canvas[, rect]) on a {width, height, format, matrix, data} video writes the expected canvas, through the
 *     addon's drawFramesYuvDevice (never drawFramesDevice);
 *  2. ccv.DeviceBatch with opts.source + sourceFormat / sourceMatrix: uploadSource + draw + whitebalance / detectStep on the drawn set,
 *     draw with a rect, drawBound + the step functions at set = -1, a refused rect, and the addon's host form drawFramesYuv.
 * Prints "ingest_yuv_gpu: ok" or the failed checks. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));
const pack = require(path.join(root, 'headtrackr_amd', 'js', 'cascade_pack.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const errors = [];
let checks = 0;
function check(cond, msg) { checks++; if (!cond && errors.length < 20) errors.push(msg); return cond; }
function same(a, b) { if (a.length !== b.length) return false; for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false; return true; }
const n = job.n, fb = job.w * job.h * 4, fsz = job.sw * job.sh + 2 * ((job.sw + 1) >> 1) * ((job.sh + 1) >> 1);

let yuvDraws = 0, rgbaDraws = 0;
const realYuv = A.drawFramesYuvDevice, realRgba = A.drawFramesDevice;
check(typeof realYuv === 'function' && typeof A.drawFramesYuv === 'function' && A.YUV_NV12 === 0 && A.YUV_I420 === 1, 'addon exports');
A.drawFramesYuvDevice = function () { yuvDraws++; return realYuv.apply(this, arguments); };
A.drawFramesDevice = function () { rgbaDraws++; return realRgba.apply(this, arguments); };

function bestIs(best, want, what) {
  for (let f = 0; f < n; f++) ['x', 'y', 'width', 'height', 'confidence'].forEach(function (k, i) { check(best[6 * f + i] === want[f][k], what + ': best[' + f + '].' + k + ' ' + best[6 * f + i] + ' != ' + want[f][k]); });
}

job.videos.forEach(function (v) {
  const data = new Uint8Array(fs.readFileSync(path.join(job.dir, v.file)));
  const want = new Uint8Array(fs.readFileSync(path.join(job.dir, v.want))), wantRect = new Uint8Array(fs.readFileSync(path.join(job.dir, v.want_rect)));
  const tag = v.format + '/' + v.matrix;
  /* 1. ccv.drawFrames */
  [null, job.rect].forEach(function (rect) {
    for (let f = 0; f < n; f++) {
      const video = { width: job.sw, height: job.sh, format: v.format, matrix: v.matrix, data: data.subarray(f * fsz, (f + 1) * fsz) };
      const dev = new Canvas(job.w, job.h), before = yuvDraws;
      headtrackr.ccv.drawFrames(video, dev, rect || undefined);
      check(yuvDraws === before + 1, tag + ': ccv.drawFrames did not take the YUV device route');
      check(same(dev.pixels, (rect ? wantRect : want).subarray(f * fb, (f + 1) * fb)), tag + ': ccv.drawFrames bytes, frame ' + f + (rect ? ' with rect' : ''));
    }
  });
  /* 2. DeviceBatch */
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 2, source: { width: job.sw, height: job.sh, sets: 2 }, sourceFormat: v.format, sourceMatrix: v.matrix });
  b.uploadSource(data, 1);
  b.draw(1, 1);
  const wb = b.whitebalance(1);
  check(wb[0] === v.wb[0] && wb[1] === v.wb[1], tag + ': whitebalance of the drawn set');
  bestIs(b.detectStep(1).best, v.best, tag + ': detectStep on the drawn set');
  b.draw(1, 0, Int32Array.from(job.rect));
  const wr = b.whitebalance(0);
  check(wr[0] === v.wb_rect[0] && wr[1] === v.wb_rect[1], tag + ': whitebalance of the set drawn with a rect');
  b.drawBound(1);
  bestIs(b.detectStep(-1).best, v.best, tag + ': detectStep(-1) after drawBound');
  const wbb = b.whitebalance(-1);
  check(wbb[0] === v.wb[0] && wbb[1] === v.wb[1], tag + ': whitebalance after drawBound');
  let threw = false;
  try { b.draw(1, 0, Int32Array.from([0, 0, job.sw + 1, job.sh])); } catch (e) { threw = /status -1/.test(e.message); }
  check(threw, tag + ': a rect outside the source frame is refused with HT_ERR_INVALID');
  b.draw(1, 0);
  const wa = b.whitebalance(0);
  check(wa[0] === v.wb[0] && wa[1] === v.wb[1], tag + ': usable after the refused draw');
  b.destroy();
  /* the addon's host form, bound */
  const c = A.createContext({ cascade: pack.packCascade(headtrackr.cascade), interval: 5, device: 0 });
  A.setGeometry(c, job.w, job.h, n, null);
  A.drawFramesYuv(c, data, n, job.sw, job.sh, v.format === 'nv12' ? A.YUV_NV12 : A.YUV_I420, ['bt601', 'bt709', 'bt601-full', 'bt709-full'].indexOf(v.matrix), null);
  const wh = A.whitebalanceBound(c, n);
  check(A.framesBound(c) === n && wh[0] === v.wb[0] && wh[1] === v.wb[1], tag + ': drawFramesYuv binds the drawn frames');
  A.destroy(c);
});
check(rgbaDraws === 0, 'a YUV source reached the RGBA entry point');

process.stdout.write(errors.length ? JSON.stringify({ ok: false, checks: checks, errors: errors }) + '\n' : 'ingest_yuv_gpu: ok (' + checks + ' checks)\n', function () { headtrackr.exitNow(errors.length ? 1 : 0); });
